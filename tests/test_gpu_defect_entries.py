"""Every entry of the defect blocks the device writes, against 50 digits, with a bound per entry (tests/defect_checker.py; fixtures:
tests/golden/defect_entries/, made by tests/golden/make_golden_defect_entries.py).  Through the C ABI as every parity test.

* every shape (the 36 library shapes, the run-time compiled families that reach kernels no library shape reaches), every evaluation
  kind: the fixture's segments as a mesh of their own;
* every launch form, by tiling: the kernels read the solver vectors only through the index tables
  (test_gpu_parity.py: test_renumbered_variables_give_the_same_blocks), so segment s of a mesh of n segments points at fixture segment
  pi(s) -- a fixed pseudo-random map in which no two neighbours are equal -- and every block of every segment is checked.  n comes
  from the launch planner: for each distinct sequence of kernel slot names (and XCD placement of the unit stage) up to 32 768
  segments the smallest size that plans it, that size minus one and a size that leaves a ragged last group;
* the assembled path at one size: the values of eval_assembled against the scatter of the blocks just checked (every other size, kernel
  and map: tests/test_gpu_assembled_entries.py).

On a 256-CU device the planner reaches every form of the tiled shapes at or below 24 577 segments (the last: K_RESL2 of
Reentry-Trapezoidal), so none is left to test_gpu_parity.py: test_launch_form_boundaries alone; on a device with more compute units a
form that starts beyond 32 768 segments would be.
The worst |got - ref| / bound of every shape and form is printed (pytest -s)."""
import functools

import numpy as np
import pytest

import defect_checker as dc
from asset_asrl_amd import _lib, jit
from asset_asrl_amd.evaluator import CON, CON_ADJGRAD, JAC, JAC_ADJGRAD, JAC_ADJGRAD_HESS, DefectEvaluator

pytestmark = pytest.mark.gpu

SHAPES = dc.all_shapes()
IDS = [dc.shape_name(*s) for s in SHAPES]
KIND_NAMES = {CON: "CON", CON_ADJGRAD: "CON_ADJGRAD", JAC: "JAC", JAC_ADJGRAD: "JAC_ADJGRAD", JAC_ADJGRAD_HESS: "JAC_ADJGRAD_HESS"}
MAX_NSEG = 32768


def device_name(ode: str, mode: str, blocked: bool) -> str:
    """The name the device code of a shape is registered under: a library ODE's own, a run-time compiled one's after compiling it
    (from the module cache the build leaves) as tests/test_gpu_shapes.py does."""
    if ode in ("brachistochrone", "reentry", "twobody_lt", "betts_lowthrust", "synthetic32"):
        return ode
    from helpers import make_coupled12, make_driven, make_shape
    if ode == "coupled12":
        return jit.ensure_kernel(make_coupled12(), mode, blocked)
    if ode == "driven14":
        return jit.ensure_kernel(make_driven(14), mode, blocked)
    n, m, p = (int(v) for v in ode.split("_")[1:])
    return jit.ensure_kernel(make_shape(n, m, p), mode, blocked)


def tiling(n: int, ns: int, seed: int = 5) -> np.ndarray:
    """pi[n]: mesh segment -> fixture segment, pseudo-random, pi(s) != pi(s + 1)"""
    if ns == 1:
        return np.zeros(n, dtype=np.int64)
    step = 1 + np.random.default_rng(seed).integers(0, ns - 1, n)          # 1 ... ns - 1: never back onto the same segment
    return np.cumsum(step) % ns


class Mesh:
    """n segments over the fixture's segment inputs: X / L hold every fixture segment once (behind a variable / row offset), Vindex /
    Cindex row s names fixture segment pi(s)."""

    def __init__(self, f, pi, var_offset=3, con_offset=2, extra_vars=4, private_last=False, private_rows=False):
        ns, IR, OR = f["x"].shape[0], f["IR"], f["OR"]
        self.pi = np.asarray(pi, dtype=np.int64)
        rng = np.random.default_rng(9)
        x, lam = f["x"], f["lam"]
        if private_last:                                   # the last segment reads a copy of its inputs that no other segment names
            x, lam = np.concatenate([x, x[self.pi[-1:]]]), np.concatenate([lam, lam[self.pi[-1:]]])
        if private_rows:                                   # every segment has constraint rows of its own, as the defects of a phase have
            lam = f["lam"][self.pi]
        self.n_primal, self.n_equal = var_offset + x.size + extra_vars, con_offset + lam.size
        self.X, self.L = rng.uniform(-1, 1, self.n_primal), rng.uniform(-1, 1, self.n_equal)
        self.X[var_offset:var_offset + x.size] = x.ravel()
        self.L[con_offset:con_offset + lam.size] = lam.ravel()
        where = self.pi.copy()
        if private_last:
            where[-1] = ns
        self.vindex = (var_offset + where[:, None] * IR + np.arange(IR)[None, :]).astype(np.int32)
        rows = np.arange(self.pi.size) if private_rows else where
        self.cindex = (con_offset + rows[:, None] * OR + np.arange(OR)[None, :]).astype(np.int32)


def check_eval(ev, f, mesh, what, slots, report):
    """One evaluation of kind ``what``: every output against the fixture.  -> the blocks (canonical order) or None"""
    hslot, jslot = slots
    fx, agx, kkt = ev.eval(what, mesh.X, mesh.L if what in (CON_ADJGRAD, JAC_ADJGRAD, JAC_ADJGRAD_HESS) else None)
    parts = [("fx", fx)]
    if agx is not None:
        parts.append(("gx", agx))
    if kkt is not None:
        parts.append(("jx", kkt[:, jslot.ravel()]))
        if what == JAC_ADJGRAD_HESS:
            parts.append(("hx", kkt[:, hslot]))
        else:
            assert not np.any(kkt[:, hslot]), "Hessian slots of a Jacobian kind must be exactly zero"
    for kind, got in parts:
        r = dc.check(got, f, mesh.pi, kind)
        report.append((KIND_NAMES[what], kind, r))
    return kkt


def assert_report(tag, report):
    worst = {}
    for what, kind, r in report:
        worst[kind] = max(worst.get(kind, 0.0), r["worst"])
    print(f"[defect entries] {tag}: worst |got - ref| / bound  " + "  ".join(f"{k} {worst[k]:.3g}" for k in dc.KINDS if k in worst))
    bad = [(what, kind, r) for what, kind, r in report if r["over"]]
    assert not bad, (tag, bad)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_shape_every_kind(shape):
    ode, mode, blocked = shape
    f = dc.load(shape)
    mesh = Mesh(f, np.arange(f["x"].shape[0]))
    ev = DefectEvaluator(device_name(*shape), mode, blocked, mesh.vindex, mesh.cindex, mesh.n_primal, mesh.n_equal)
    assert (ev.IR, ev.OR) == (f["IR"], f["OR"])
    slots = dc.block_slots(ev.IR, ev.OR)
    report = []
    for what in (JAC_ADJGRAD_HESS, JAC, JAC_ADJGRAD, CON, CON_ADJGRAD):
        check_eval(ev, f, mesh, what, slots, report)
    ev.close()
    assert_report(dc.shape_name(*shape), report)


@functools.lru_cache(maxsize=None)
def planned_forms(name, mode, blocked, cus, what=JAC_ADJGRAD_HESS, max_nseg=MAX_NSEG, assembled=False):
    """{form: [sizes]} from the planner (``assembled``: of the evaluation into a value array, tests/test_gpu_assembled_entries.py): form = (kernel slot names ..., XCD placement of the unit stage); sizes = the smallest that
    plans it, that size minus one, one that is no multiple of the plan's group -- the segments per group of a unit stage, else the
    number of workgroups the mesh is split over -- (the first with more than two groups of it where the form has such a size)."""
    first, group_of = {}, {}
    order = []
    for n in range(1, max_nseg + 1):
        steps, units_gp = _lib.launch_plan(name, _lib.MODES[mode], blocked, what, assembled, n, cus=cus)
        form = tuple(s[0] for s in steps) + (("xcd",) if units_gp > 0 else ())
        if form not in first:
            first[form] = n
            order.append(form)
        g = max(s[6] for s in steps)                       # segments per group of a unit stage; the other kernels split the mesh
        group_of.setdefault(form, []).append((n, g if g > 0 else steps[-1][1]))   # over the workgroups of their grid
    out = {}
    for form in order:
        sizes = [first[form]] + ([first[form] - 1] if first[form] > 1 else [])
        ragged = [(n, g) for n, g in group_of[form] if g > 1 and n % g and n > first[form]]
        pick = [n for n, g in ragged if n > 2 * g] or [n for n, g in ragged]
        if pick:
            sizes.append(pick[0])
        out[form] = sizes
    return out


TILED = [("reentry", "LGL7", False), ("reentry", "LGL3", False), ("twobody_lt", "LGL5", True), ("twobody_lt", "LGL7", False),
         ("betts_lowthrust", "LGL5", False), ("betts_lowthrust", "LGL7", False), ("brachistochrone", "LGL7", False),
         ("reentry", "Trapezoidal", False), ("synthetic32", "LGL7", False), ("coupled12", "LGL7", False), ("driven14", "LGL7", False)]


def device_cus() -> int:
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def run_tiled(shape, name, f, n, forms_seen, whats, report_tag, keep_blocks=False, private_last=False, private_rows=False):
    mode, blocked = shape[1], shape[2]
    mesh = Mesh(f, tiling(n, f["x"].shape[0]), private_last=private_last, private_rows=private_rows)
    ev = DefectEvaluator(name, mode, blocked, mesh.vindex, mesh.cindex, mesh.n_primal, mesh.n_equal)
    slots = dc.block_slots(ev.IR, ev.OR)
    report, blocks = [], None
    for what in whats:
        planned = _lib.launch_plan(name, _lib.MODES[mode], blocked, what, False, n, cus=device_cus())
        assert ev.launch_plan(what) == planned, (n, what)                   # the handle launches what was planned
        forms_seen.add(tuple(s[0] for s in planned[0]))
        kkt = check_eval(ev, f, mesh, what, slots, report)
        if what == JAC_ADJGRAD_HESS and keep_blocks:
            blocks = kkt
    assert_report(report_tag, report)
    return ev, mesh, blocks


@pytest.mark.parametrize("shape", TILED, ids=[dc.shape_name(*s) for s in TILED])
def test_every_launch_form_by_tiling(shape):
    f = dc.load(shape)
    name = device_name(*shape)
    cus = device_cus()
    if shape[0] == "synthetic32":                          # (wide blocks: 1, 3 and 257 segments -- fewer than workgroups, unequal shares)
        plan = {("K_LGL2_S1", "K_ROWS2"): [1, 3, 257]}
    else:
        plan = planned_forms(name, shape[1], shape[2], cus)
    seen = set()
    for form, sizes in plan.items():
        for i, n in enumerate(sizes):
            whats = (JAC_ADJGRAD_HESS, JAC, CON_ADJGRAD) if i == 0 else (JAC_ADJGRAD_HESS,)
            ev, _, _ = run_tiled(shape, name, f, n, seen, whats, f"{dc.shape_name(*shape)} {'+'.join(form)} x{n}")
            ev.close()
    # which forms this device was held on, at which sizes (a form with two sizes has none with a ragged last group up to MAX_NSEG)
    print(f"[defect entries] {dc.shape_name(*shape)} on {cus} compute units: "
          + "; ".join(f"{'+'.join(form)} x{sizes}" for form, sizes in plan.items())
          + "; kernels launched: " + ", ".join(sorted({k for form in seen for k in form})))
    assert {tuple(k for k in form if k != "xcd") for form in plan} <= seen, (plan, seen)   # every planned form did run
    if cus == 256:                                         # what the shapes are here for: the forms a 256-CU device takes
        want = {("reentry", "LGL7"): {"K_RES2", "K_RES_ALT", "K_RESLP"}, ("twobody_lt", "LGL5"): {"K_RES2", "K_RESL2"},
                ("betts_lowthrust", "LGL5"): {"K_UNITS4", "K_RESD"}, ("betts_lowthrust", "LGL7"): {"K_RESD"},
                ("driven14", "LGL7"): {"K_ROWS2"}}.get(shape[:2], set())
        assert want <= {s for form in seen for s in form}, (want, seen)


def test_assembled_values_are_the_scatter_of_the_checked_blocks(oracle):
    """Reentry-LGL7 at the smallest size of the row-wise form: eval_assembled against the scatter of blocks the fixture has just held
    entry by entry.  With a map set the planner never takes the row-wise form -- at this size the block path launches K_RES_ALT, the
    assembled path the tile form K_RES2_ASM -- and two forms agree only to rounding (on an MI355X with 256 compute units: up to 211 x 4 u sum |c| between the
    two).  So the blocks that are scattered are the assembled path's own: the same handle under a map that gives every slot a location
    of its own, held to the fixture like every other block; then the mesh's real map.  The tiled mesh shares every variable between
    many segments, so many blocks add into one Hessian location in an order that is not known: within 4 u sum |contributions| per
    location; bit for bit where a location takes one.  Every segment keeps constraint rows of its own, as the defects of a phase
    do: a Jacobian location then takes one contribution (the map builder adds the slots of a shared Jacobian location atomically,
    one after the other, and 439 terms in an unknown order are only held by 438 u sum |c|: 26 x 4 u sum |c| with shared rows on that device.  What this test
    leaves open -- the other assembly kernels, shared locations held harder than 4 u sum |c|, many-way Jacobian sums, the staged
    reduction, the RHS gathers -- is held per location by tests/test_gpu_assembled_entries.py)."""
    shape = ("reentry", "LGL7", False)
    f = dc.load(shape)
    cus = device_cus()
    forms = planned_forms("reentry", "LGL7", False, cus)
    rows = [sizes[0] for form, sizes in forms.items() if "K_RES_ALT" in form]
    assert rows, forms
    n = rows[0]
    ev, mesh, _ = run_tiled(shape, "reentry", f, n, set(), (JAC_ADJGRAD_HESS,), f"reentry_LGL7 blocks x{n}", private_last=True,
                            private_rows=True)
    planned = _lib.launch_plan("reentry", _lib.MODES["LGL7"], False, JAC_ADJGRAD_HESS, True, n, cus=cus)
    assert ev.launch_plan(JAC_ADJGRAD_HESS, assembled=True) == planned
    # the assembled path's blocks: every slot its own location
    ev.set_kkt_map(np.arange(n * ev.NKKT, dtype=np.int32).reshape(n, ev.NKKT), n * ev.NKKT)
    blocks = np.zeros(n * ev.NKKT)
    fx, agx = ev.eval_assembled(JAC_ADJGRAD_HESS, mesh.X, mesh.L, blocks)
    blocks = blocks.reshape(n, ev.NKKT)
    hslot, jslot = dc.block_slots(ev.IR, ev.OR)
    report = [("ASSEMBLED", kind, dc.check(got, f, mesh.pi, kind))
              for kind, got in (("fx", fx), ("gx", agx), ("jx", blocks[:, jslot.ravel()]), ("hx", blocks[:, hslot]))]
    assert_report(f"reentry_LGL7 {'+'.join(s[0] for s in planned[0])} x{n}", report)
    # the mesh's own map
    nlp = oracle.Nlp(oracle.get_ode("reentry", 0), oracle.MODES["LGL7"], False, mesh.vindex, mesh.cindex, mesh.n_primal, mesh.n_equal, 2)
    locs = nlp.kkt_locations()[:nlp.num_user_kkt].reshape(n, ev.NKKT)
    # (a mesh tiled from six segments has no location with a single contribution: the last segment has variables of its own)
    ev.set_kkt_map(locs, nlp.nnz)
    vals = np.zeros(nlp.nnz)
    ev.eval_assembled(JAC_ADJGRAD_HESS, mesh.X, mesh.L, vals)
    flat = locs.ravel()
    count = np.bincount(flat, minlength=nlp.nnz)
    total = np.zeros(nlp.nnz, dtype=np.longdouble)
    np.add.at(total, flat, blocks.ravel().astype(np.longdouble))
    mag = np.bincount(flat, weights=np.abs(blocks.ravel()), minlength=nlp.nnz)
    err = np.abs(vals - total).astype(np.float64)
    many = count > 1
    ratio = np.divide(err, 4.0 * dc.U * mag, out=np.zeros_like(err), where=mag > 0)
    single = count == 1
    print(f"[defect entries] reentry_LGL7 assembled x{n}: {int(many.sum())} shared locations, up to {int(count.max())} contributions, "
          f"worst |assembled - scatter| / (4 u sum|c|) = {ratio[many].max():.3g}; {int(single.sum())} single locations, "
          f"{int(np.sum(vals[single] != total[single].astype(np.float64)))} of them not bit for bit")
    assert np.all(vals[count == 0] == 0.0) and single.sum() >= ev.NKKT - ev.IR * ev.OR
    assert np.array_equal(vals[single], total[single].astype(np.float64))
    assert np.all(err[many] <= 4.0 * dc.U * mag[many])
    ev.close()
