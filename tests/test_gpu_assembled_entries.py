"""Every value the on-device KKT assembly leaves in the solver's value array, and every entry the RHS gathers add to FXE / AGX, per
location (tests/assembled_checker.py; fixtures: tests/golden/defect_entries/).  Through the C ABI, as tests/test_gpu_defect_entries.py,
whose meshes and helpers these tests use.

a. every fixture shape, every kind with KKT entries: a permuted map that gives every slot a location of its own -- the assembled
   path's blocks, held entry by entry like the stored ones;
b. every assembled launch form by tiling, sizes from the planner; the looped forms on the shape where they start smallest;
c. maps BY CONSTRUCTION (assembled_checker.CONSTRUCTED) in the default mode: given the blocks of the same handle, every location with
   one slot, two slots, or three and more Hessian slots (staged, asm_reduce_kernel) is held BIT FOR BIT, many-way Jacobian sums within
   (k - 1) u sum |c|, everything inside the 50-digit bound of its location; through the device entry and both host entries;
d. accumulate mode into a random base, twice;
e. the RHS gathers of asset_hip_defect_eval_kkt_device on a mesh with 1, 2, 64, 65, 256 and 257 contributors per row: bit for bit the
   restated gather of the blocks, inside the bound of the fixture, repeatable.
Worst ratios and the wall time of every case are printed (pytest -s)."""
import time

import numpy as np
import pytest
import torch

import assembled_checker as ac
import defect_checker as dc
from asset_asrl_amd import _lib
from asset_asrl_amd.evaluator import CON, CON_ADJGRAD, JAC, JAC_ADJGRAD, JAC_ADJGRAD_HESS, DefectEvaluator
from test_gpu_defect_entries import (IDS, KIND_NAMES, MAX_NSEG, SHAPES, TILED, Mesh, assert_report, device_cus, device_name,
                                     planned_forms, tiling)

pytestmark = pytest.mark.gpu

KKT_KINDS = (JAC_ADJGRAD_HESS, JAC, JAC_ADJGRAD)
SENTINEL = -1234.5678                                      # finite: a kernel that adds to it shows, one that stores over it shows
LOOPED = ("K_RESL1_ASM", "K_RESL2_ASM")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def evaluator(shape, name, mesh):
    return DefectEvaluator(name, shape[1], shape[2], mesh.vindex, mesh.cindex, mesh.n_primal, mesh.n_equal)


def run_device(ev, what, mesh, prefill, times=1):
    """eval_assembled_device into a device array that holds ``prefill``.  -> (fx blocks, agx blocks or None, values)"""
    X, L = dev(mesh.X), (dev(mesh.L) if what != JAC else None)
    fx = torch.full((ev.nseg * ev.OR,), float("nan"), dtype=torch.float64, device="cuda:0")
    agx = torch.full((ev.nseg * ev.IR,), float("nan"), dtype=torch.float64, device="cuda:0") if what != JAC else None
    vals = dev(prefill)
    torch.cuda.synchronize()                               # (torch fills on its stream, the evaluator runs on its own)
    for _ in range(times):
        ev.eval_assembled_device(what, X, L, fx, agx, vals)
    torch.cuda.synchronize()
    return (fx.cpu().numpy().reshape(ev.nseg, ev.OR), None if agx is None else agx.cpu().numpy().reshape(ev.nseg, ev.IR),
            vals.cpu().numpy())


def check_own_locations(ev, f, mesh, what, locs, nvalues, report):
    """One assembled evaluation under a map that gives every slot a location of its own: every entry against the fixture; for the
    Jacobian kinds the Hessian locations keep a sentinel.  -> (fx, agx, blocks[nseg, NKKT] canonical order)"""
    hslot, jslot = dc.block_slots(ev.IR, ev.OR)
    prefill = np.zeros(nvalues)
    if what != JAC_ADJGRAD_HESS:
        prefill[locs[:, hslot].ravel()] = SENTINEL
    fx, agx, vals = run_device(ev, what, mesh, prefill)
    blocks = vals[locs]
    parts = [("fx", fx), ("jx", blocks[:, jslot.ravel()])]
    if agx is not None:
        parts.append(("gx", agx))
    if what == JAC_ADJGRAD_HESS:
        parts.append(("hx", blocks[:, hslot]))
    else:
        assert np.all(blocks[:, hslot] == SENTINEL), "a Jacobian kind touched a Hessian location"
    for kind, got in parts:
        report.append((KIND_NAMES[what], kind, dc.check(got, f, mesh.pi, kind)))
    return fx, agx, blocks


def planned(ev, name, shape, what, cus):
    plan = _lib.launch_plan(name, _lib.MODES[shape[1]], shape[2], what, True, ev.nseg, cus=cus)
    assert ev.launch_plan(what, assembled=True) == plan, (ev.nseg, what)        # the handle launches what was planned
    return tuple(s[0] for s in plan[0])


# ---- a. every shape, every kind ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_shape_every_kind_assembled(shape):
    t0 = time.perf_counter()
    f = dc.load(shape)
    name = device_name(*shape)
    mesh = Mesh(f, np.arange(f["x"].shape[0]))
    ev = evaluator(shape, name, mesh)
    locs, nvalues = ac.make_map(ev.nseg, ev.IR, ev.OR, {}, 21)
    assert np.unique(locs).size == locs.size == nvalues
    ev.set_kkt_map(locs, nvalues)
    report, seen = [], set()
    for what in KKT_KINDS:
        seen.add(planned(ev, name, shape, what, device_cus()))
        check_own_locations(ev, f, mesh, what, locs, nvalues, report)
    ev.close()
    assert_report(f"{dc.shape_name(*shape)} assembled {sorted('+'.join(s) for s in seen)}", report)
    print(f"[assembled entries] {dc.shape_name(*shape)}: {time.perf_counter() - t0:.2f} s")


# ---- b. every assembled launch form ---------------------------------------------------------------------------------------------------
def run_tiled_assembled(shape, name, f, n, whats, seen, tag):
    t0 = time.perf_counter()
    mesh = Mesh(f, tiling(n, f["x"].shape[0]))
    ev = evaluator(shape, name, mesh)
    locs, nvalues = ac.segment_permuted_map(n, ev.NKKT, 7)
    ev.set_kkt_map(locs, nvalues)
    report = []
    for what in whats:
        seen.add(planned(ev, name, shape, what, device_cus()))
        check_own_locations(ev, f, mesh, what, locs, nvalues, report)
    ev.close()
    assert_report(f"{tag} x{n} assembled", report)
    print(f"[assembled entries] {tag} x{n}: {time.perf_counter() - t0:.2f} s")


def looped_shape(kernel, cus):
    """(first size x NKKT, shape, sizes) of the shape on which ``kernel`` starts at the smallest value array, from the planner"""
    what = JAC if kernel == "K_RESL1_ASM" else JAC_ADJGRAD_HESS
    best = None
    for shape in [s for s in TILED if s[0] in dc.LIBRARY_ODES] + [("reentry", "LGL5", False)]:
        f = dc.load(shape)
        nk = f["IR"] * (f["IR"] + 1) // 2 + f["OR"] * f["IR"]
        for form, sizes in planned_forms(shape[0], shape[1], shape[2], cus, what=what, assembled=True).items():
            if kernel in form and (best is None or sizes[0] * nk < best[0]):
                best = (sizes[0] * nk, shape, sizes)
    return best


@pytest.mark.parametrize("shape", TILED + [("synthetic32", "Trapezoidal", False)],
                         ids=[dc.shape_name(*s) for s in TILED] + ["synthetic32_Trapezoidal"])
def test_every_assembled_launch_form_by_tiling(shape):
    """The looped forms are held where they start at the smallest value array (test_looped_assembly_forms); here they are printed."""
    f = dc.load(shape)
    name = device_name(*shape)
    cus = device_cus()
    if shape[0] == "synthetic32":                          # (wide blocks: 1, 3 and 257 segments -- fewer than workgroups, unequal shares)
        form = tuple(s[0] for s in _lib.launch_plan(name, _lib.MODES[shape[1]], shape[2], JAC_ADJGRAD_HESS, True, 1, cus=cus)[0])
        plan = {form: [1, 3, 257] if shape[1] == "LGL7" else [1, 3, 77]}
    else:
        plan = planned_forms(name, shape[1], shape[2], cus, assembled=True)
    left = {form: sizes for form, sizes in plan.items() if set(form) & set(LOOPED)}
    plan = {form: sizes for form, sizes in plan.items() if form not in left}
    beyond = {}                                            # forms that only start beyond MAX_NSEG segments: named, not held
    for n in [1 << k for k in range(16, 23)] + [4000000]:
        steps, gp = _lib.launch_plan(name, _lib.MODES[shape[1]], shape[2], JAC_ADJGRAD_HESS, True, n, cus=cus)
        form = tuple(s[0] for s in steps) + (("xcd",) if gp > 0 else ())
        if form not in plan and form not in left:
            beyond.setdefault(form, n)
    seen = set()
    for form, sizes in plan.items():
        for i, n in enumerate(sizes):
            run_tiled_assembled(shape, name, f, n, KKT_KINDS if i == 0 else (JAC_ADJGRAD_HESS,), seen,
                                f"{dc.shape_name(*shape)} {'+'.join(form)}")
    print(f"[assembled entries] {dc.shape_name(*shape)} on {cus} compute units: "
          + "; ".join(f"{'+'.join(form)} x{sizes}" for form, sizes in plan.items())
          + "; kernels launched: " + ", ".join(sorted({k for form in seen for k in form}))
          + "".join(f"; {'+'.join(form)} (from {sizes[0]}) is held on {dc.shape_name(*looped_shape('K_RESL2_ASM', cus)[1])}"
                    for form, sizes in left.items())
          + "".join(f"; NOT HELD, starts beyond {MAX_NSEG} segments: {'+'.join(form)} (planned at {n})" for form, n in beyond.items()))
    assert {tuple(k for k in form if k != "xcd") for form in plan} <= seen, (plan, seen)   # every planned form did run
    if cus == 256:                                         # what the shapes are here for: the forms a 256-CU device takes
        want = {("reentry", "LGL7"): {"K_RES1_ASM", "K_RES2_ASM"}, ("twobody_lt", "LGL7"): {"K_LGL1_S3_ASM", "K_LGL2_S3_ASM"},
                ("betts_lowthrust", "LGL5"): {"K_RESD_ASM"}, ("synthetic32", "LGL7"): {"K_WIDE1_ASM", "K_WIDE2_ASM"},
                ("synthetic32", "Trapezoidal"): {"K_LGL1_S2_ASM", "K_LGL2_S2_ASM"}}.get(shape[:2], set())
        assert want <= {s for form in seen for s in form}, (want, seen)


@pytest.mark.parametrize("kernel", LOOPED)
def test_looped_assembly_forms(kernel):
    cus = device_cus()
    best = looped_shape(kernel, cus)
    assert best is not None, f"no shape plans {kernel} up to {MAX_NSEG} segments on {cus} compute units"
    _, shape, sizes = best
    f = dc.load(shape)
    seen = set()
    for n in sizes:
        whats = (JAC, JAC_ADJGRAD) if kernel == "K_RESL1_ASM" else (JAC_ADJGRAD_HESS,)
        run_tiled_assembled(shape, shape[0], f, n, whats, seen, f"{dc.shape_name(*shape)} {kernel}")
    assert kernel in {k for form in seen for k in form}, seen


# ---- c. constructed maps, default mode ---------------------------------------------------------------------------------------------
def own_blocks(ev, f, mesh, tag):
    """The assembled path's own blocks: the handle under a map that gives every slot a location of its own, held by the fixture."""
    own, nown = ac.segment_permuted_map(ev.nseg, ev.NKKT, 5)
    ev.set_kkt_map(own, nown)
    report = []
    fx, agx, blocks = check_own_locations(ev, f, mesh, JAC_ADJGRAD_HESS, own, nown, report)
    assert_report(tag + " blocks", report)
    return fx, agx, blocks


def location_report(tag, vals, ref, bnd, cnt, exact):
    res = ac.check_sum(vals[cnt > 0], ref[cnt > 0], bnd[cnt > 0])
    print(f"[assembled entries] {tag}: worst |got - ref| / bound {res['worst']:.3g} over {res['n']} locations, {int(exact.sum())} held "
          f"bit for bit, {int((cnt > 0).sum() - exact.sum())} by a bound of their own sum, largest class {int(cnt.max())}")
    assert res["over"] == 0, (tag, res)


@pytest.mark.parametrize("case", ac.CONSTRUCTED, ids=[ac.constructed_id(c) for c in ac.CONSTRUCTED])
def test_constructed_map_default_mode(case):
    t0 = time.perf_counter()
    shape, nseg, _, seed = case
    tag = ac.constructed_id(case)
    f = dc.load(shape)
    mesh = Mesh(f, tiling(nseg, f["x"].shape[0]))
    ev = evaluator(shape, device_name(*shape), mesh)
    fx, agx, blocks = own_blocks(ev, f, mesh, tag)
    locs, nvalues = ac.constructed_map(case)
    ev.set_kkt_map(locs, nvalues)
    exp, tol, cnt, staged = ac.expected_values(locs, nvalues, blocks, ev.IR, ev.OR)
    exact, used, loose = (tol == 0) & (cnt > 0), cnt > 0, tol > 0
    lo, hi = int(np.nonzero(used)[0][0]), int(np.nonzero(used)[0][-1]) + 1
    r, b = ac.fixture_blocks(f, mesh.pi)
    ref, bnd, _ = ac.sum_reference(locs, r, b, nvalues)
    # the device entry: zeros where the constraint has a slot (the contract of the default map), a sentinel everywhere else
    fx2, agx2, vals = run_device(ev, JAC_ADJGRAD_HESS, mesh, np.where(used, 0.0, SENTINEL))
    assert np.array_equal(fx2, fx) and np.array_equal(agx2, agx)
    assert np.all(vals[~used] == SENTINEL), "a location no slot names was written"
    for k, which in (("one slot", cnt == 1), ("two slots", cnt == 2), ("staged", staged)):
        bad = np.nonzero(which & (vals != exp))[0]
        assert bad.size == 0, (tag, k, bad[:5], vals[bad[:5]], exp[bad[:5]])
    assert np.all(np.abs(vals - exp)[loose] <= tol[loose])
    location_report(tag, vals, ref, bnd, cnt, exact)
    # the host entries: added onto what the caller's array holds / copied over a cleared range
    base = np.random.default_rng(seed).uniform(-1, 1, nvalues)
    out = base.copy()
    hfx, hagx = ev.eval_assembled(JAC_ADJGRAD_HESS, mesh.X, mesh.L, out)
    assert np.array_equal(hfx, fx) and np.array_equal(hagx, agx)
    want = base + exp                                      # (exp is 0 where nothing is written: base + 0 = base)
    assert np.array_equal(out[~used], base[~used]) and np.array_equal(out[exact], want[exact])
    assert np.all(np.abs(out - want)[loose] <= tol[loose] + ac.U * np.abs(want[loose]))
    out = np.full(nvalues, SENTINEL)
    ev.eval_assembled(JAC_ADJGRAD_HESS, mesh.X, mesh.L, out, target_zeroed=True)
    assert np.all(out[:lo] == SENTINEL) and np.all(out[hi:] == SENTINEL)
    inside = np.zeros(nvalues, dtype=bool)
    inside[lo:hi] = True
    assert np.array_equal(out[inside & (tol == 0)], exp[inside & (tol == 0)])           # (gaps inside the range: cleared)
    assert np.all(np.abs(out - exp)[loose] <= tol[loose])
    ev.close()
    print(f"[assembled entries] {tag}: {time.perf_counter() - t0:.2f} s")


# ---- d. accumulate mode ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in ac.CONSTRUCTED if c[1] == 7], ids=[ac.constructed_id(c) for c in ac.CONSTRUCTED if c[1] == 7])
def test_constructed_map_accumulate_mode(case):
    t0 = time.perf_counter()
    shape, nseg, _, seed = case
    f = dc.load(shape)
    mesh = Mesh(f, tiling(nseg, f["x"].shape[0]))
    ev = evaluator(shape, device_name(*shape), mesh)
    locs, nvalues = ac.constructed_map(case)
    ev.set_kkt_map(locs, nvalues, accumulate=True)
    base = np.random.default_rng(seed + 50).uniform(-1, 1, nvalues)
    _, _, vals = run_device(ev, JAC_ADJGRAD_HESS, mesh, base, times=2)
    ev.close()
    r, b = ac.fixture_blocks(f, mesh.pi)
    ref, sb, sa, cnt = ac.sum_parts(locs, r, b, nvalues)
    assert np.array_equal(vals[cnt == 0], base[cnt == 0])
    # base + 2 k terms, each contribution twice: 2 sum b_i for the entries, (2 k) u (|base| + 2 sum (|r_i| + b_i)) for 2 k additions
    bound = 2.0 * sb + 2.0 * cnt * ac.U * (np.abs(base) + 2.0 * sa)
    want = base.astype(np.longdouble) + 2.0 * ref.astype(np.longdouble)
    used = cnt > 0
    res = ac.check_sum((vals.astype(np.longdouble) - want).astype(np.float64)[used], np.zeros(int(used.sum())), bound[used])
    print(f"[assembled entries] {ac.constructed_id(case)} accumulate, twice: worst |got - ref| / bound {res['worst']:.3g} over {res['n']} "
          f"locations; {time.perf_counter() - t0:.2f} s")
    assert res["over"] == 0, res


# ---- e. the RHS gathers ----------------------------------------------------------------------------------------------------------------
MULT = (1, 2, 64, 65, 256, 257)


def run_kkt_device(ev, what, mesh, base_fxe, base_agx, nvalues):
    X = dev(mesh.X)
    L = dev(mesh.L) if what in (CON_ADJGRAD, JAC_ADJGRAD, JAC_ADJGRAD_HESS) else None
    FXE, AGX = dev(base_fxe), (dev(base_agx) if L is not None else None)
    vals = torch.zeros(nvalues, dtype=torch.float64, device="cuda:0") if what >= JAC else None
    torch.cuda.synchronize()
    ev.eval_kkt_device(what, X, L, FXE, AGX, vals)
    torch.cuda.synchronize()
    return FXE.cpu().numpy(), None if AGX is None else AGX.cpu().numpy(), None if vals is None else vals.cpu().numpy()


def block_path(ev, what, mesh):
    """The fx / agx blocks of a value or gradient kind (no map: the evaluation eval_kkt_device launches for it)"""
    X, L = dev(mesh.X), (dev(mesh.L) if what == CON_ADJGRAD else None)
    fx = torch.full((ev.nseg * ev.OR,), float("nan"), dtype=torch.float64, device="cuda:0")
    agx = torch.full((ev.nseg * ev.IR,), float("nan"), dtype=torch.float64, device="cuda:0") if L is not None else None
    torch.cuda.synchronize()
    ev.eval_device(what, X, L, fx, agx, None)
    torch.cuda.synchronize()
    return fx.cpu().numpy().reshape(ev.nseg, ev.OR), None if agx is None else agx.cpu().numpy().reshape(ev.nseg, ev.IR)


@pytest.mark.parametrize("rows", ["private", "shared", "mixed"])
@pytest.mark.parametrize("shape", [ac.R7, ac.B5], ids=lambda s: dc.shape_name(*s))
def test_rhs_gathers(shape, rows):
    t0 = time.perf_counter()
    f = dc.load(shape)
    mesh = ac.mult_mesh(f, MULT, rows)
    assert mesh.pi.size == 645 and np.bincount(mesh.pi).tolist() == list(MULT)
    ev = evaluator(shape, shape[0], mesh)
    tag = f"{dc.shape_name(*shape)} x645 {rows} rows"
    rng = np.random.default_rng(31)
    base_fxe, base_agx = rng.uniform(-1, 1, mesh.n_equal), rng.uniform(-1, 1, mesh.n_primal)
    own, nown = ac.segment_permuted_map(ev.nseg, ev.NKKT, 5)
    for what in (JAC_ADJGRAD_HESS, CON, CON_ADJGRAD):
        if what == JAC_ADJGRAD_HESS:
            fx, agx, blocks = own_blocks(ev, f, mesh, tag)
        else:
            fx, agx = block_path(ev, what, mesh)
            report = [(KIND_NAMES[what], k, dc.check(g, f, mesh.pi, k)) for k, g in (("fx", fx), ("gx", agx)) if g is not None]
            assert_report(f"{tag} {KIND_NAMES[what]} blocks", report)
        runs = [run_kkt_device(ev, what, mesh, base_fxe, base_agx, nown) for _ in range(2)]
        for a, c in zip(*runs):
            assert (a is None and c is None) or np.array_equal(a, c), (tag, what)          # repeatable, bit for bit
        FXE, AGX, vals = runs[0]
        if vals is not None:
            assert np.array_equal(vals[own], blocks)
        for kind, got, index, blk, base in (("fx", FXE, mesh.cindex, fx, base_fxe), ("gx", AGX, mesh.vindex, agx, base_agx)):
            if got is None:
                continue
            want, n = ac.gather(index, blk, base)
            short, long_ = int(((n > 0) & (n <= ac.SHORT_ROW)).sum()), int((n > ac.SHORT_ROW).sum())
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (tag, KIND_NAMES[what], kind, bad[:5], n[bad[:5]], got[bad[:5]], want[bad[:5]])
            ids = np.repeat(mesh.pi, index.shape[1])
            col = np.tile(np.arange(index.shape[1]), mesh.pi.size)
            ref, bnd, cnt = ac.sum_reference(index, f[kind][ids, col], dc.bound(f[kind + "E"], kind)[ids, col], base.size)
            assert np.array_equal(cnt, n)
            total = base + ref                             # one more addition, of the base: u (|base| + |sum|) at the most
            res = ac.check_sum(got, total, bnd + ac.U * (np.abs(base) + np.abs(ref) + bnd))
            print(f"[assembled entries] {tag} {KIND_NAMES[what]} {kind}: {short} short rows, {long_} long rows, up to {int(n.max())} "
                  f"contributors, all bit for bit the restated gather; worst |got - ref| / bound {res['worst']:.3g}")
            assert res["over"] == 0, (tag, kind, res)
            if kind == "gx":
                assert sorted(set(n[n > 0].tolist())) == sorted(MULT)
            elif rows == "shared":
                assert sorted(set(n[n > 0].tolist())) == sorted(MULT)
            elif rows == "mixed":                          # the edge of the short grid (256 rows a block) and long rows in one gather
                assert short > 256 and long_ >= 2, (short, long_)
    ev.close()
    print(f"[assembled entries] {tag}: {time.perf_counter() - t0:.2f} s")
