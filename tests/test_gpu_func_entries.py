"""Every entry of the blocks the plain-function kernels write (csrc/func_kernels.h, reached through FunctionEvaluator and
FunctionBundle), against 50 digits, with a bound per entry (tests/func_checker.py; fixtures: tests/golden/func_entries/, made by
tests/golden/make_golden_func_entries.py).  Every evaluation goes through the device-pointer entry points of the C ABI with the
outputs pre-filled with NaN: a slot the kernel does not write cannot pass (the generated functor promises every entry, structural
zeros included; the staging of the host-pointer ``eval`` would hide a miss).

a. every function, every evaluation kind: the six fixture applications as a mesh of their own;
b. every staging class (FuncStage<F>::APW = 64, 32, 16, 8, 4 applications per workgroup staged in LDS, 0 = direct stores) at the edges
   of its copy-out loop, by tiling: application s of a mesh of n points at fixture application pi(s), pi(s) != pi(s + 1)
   (tests/test_gpu_defect_entries.py: ``tiling``, ``Mesh``), n = 1, APW - 1, APW, APW + 1, 2 APW + 1 and one n whose last group copies
   an exact multiple of 8 x 64 elements (or, where no such n exists, the nearest count above one); the launch plan is asserted before
   every evaluation;
c. bundles held to the fixture, not to separate launches: eight members in one launch -- seven that cover the six classes, each on a
   ragged mesh of 2 APW + 1 applications of its own, and one with a single application -- and the same members in reversed order;
d. the assembled forms K_FUNC1_ASM / K_FUNC2_ASM: under a map that gives every slot a location of its own the entries are held to the
   fixture; then a tiled mesh with shared variables, against the scatter of those blocks; an objective-shaped map (Jacobian slots
   dropped); the staged many-way locations twice, bit for bit.
The worst |got - ref| / bound of every function and size is printed (pytest -s)."""
import numpy as np
import pytest

import func_checker as fc
from asset_asrl_amd import jit
from asset_asrl_amd.evaluator import CON, CON_ADJGRAD, JAC, JAC_ADJGRAD, JAC_ADJGRAD_HESS, reference_slot_order
from asset_asrl_amd.pathfuncs import FunctionBundle, FunctionEvaluator
from test_gpu_defect_entries import Mesh, tiling

pytestmark = pytest.mark.gpu

NAMES = fc.all_names()
KIND_NAMES = {CON: "CON", CON_ADJGRAD: "CON_ADJGRAD", JAC: "JAC", JAC_ADJGRAD: "JAC_ADJGRAD", JAC_ADJGRAD_HESS: "JAC_ADJGRAD_HESS"}
ADJ = (CON_ADJGRAD, JAC_ADJGRAD, JAC_ADJGRAD_HESS)
SLOT = {CON: "K_FUNC0", CON_ADJGRAD: "K_FUNC1", JAC: "K_FUNC1", JAC_ADJGRAD: "K_FUNC1", JAC_ADJGRAD_HESS: "K_FUNC2"}
CLASSES_LAUNCHED = {}                                      # staging class -> [(function, sizes)] of test b, listed by the last test


def dev_tensor(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def nan_tensor(n):
    import torch
    return torch.full((int(n),), float("nan"), dtype=torch.float64, device="cuda:0")


def evaluator(f, mesh, vindex=None, n_primal=None):
    func, name = fc.product_function(f)
    ev = FunctionEvaluator(func, name, mesh.vindex if vindex is None else vindex, mesh.cindex,
                           mesh.n_primal if n_primal is None else n_primal, mesh.n_equal)
    assert (ev.IR, ev.OR, ev.NKKT) == (f["IR"], f["OR"], f["NKKT"])
    if "ac" in f:
        ev.set_appl_consts(f["ac"][mesh.pi])               # the constants of an application follow pi
    return ev


def outputs(ev, what):
    """NaN-filled device outputs of kind ``what``: (fx, agx or None, kkt or None)"""
    return (nan_tensor(ev.nseg * ev.OR), nan_tensor(ev.nseg * ev.IR) if what in ADJ else None,
            nan_tensor(ev.nseg * ev.KSTRIDE) if what in (JAC, JAC_ADJGRAD, JAC_ADJGRAD_HESS) else None)


def check_outputs(ev, f, pi, what, outs, slots, report):
    """Every output entry of one evaluation against the fixture; -> the blocks in the canonical order (or None)"""
    hslot, jslot = slots
    fx, agx, kkt = outs
    parts = [("fx", fx.cpu().numpy())]
    if agx is not None:
        parts.append(("gx", agx.cpu().numpy()))
    blocks = None
    if kkt is not None:
        blocks = ev.kkt_to_reference(kkt)
        parts.append(("jx", blocks[:, jslot.ravel()]))
        if what == JAC_ADJGRAD_HESS:
            parts.append(("hx", blocks[:, hslot]))
        else:
            assert np.all(blocks[:, hslot] == 0.0), "Hessian slots of a Jacobian kind must be exactly 0.0"
    for kind, got in parts:
        report.append((KIND_NAMES[what], kind, fc.check(got, f, pi, kind)))
    return blocks


def check_eval(ev, f, mesh, what, slots, report):
    import torch
    X, L = dev_tensor(mesh.X), dev_tensor(mesh.L)
    outs = outputs(ev, what)
    torch.cuda.synchronize()                               # (torch fills on its stream, the evaluator runs on its own)
    ev.eval_device(what, X, L if what in ADJ else None, *outs)
    torch.cuda.synchronize()
    return check_outputs(ev, f, mesh.pi, what, outs, slots, report)


def assert_report(tag, report):
    worst = {}
    for what, kind, r in report:
        worst[kind] = max(worst.get(kind, 0.0), r["worst"])
    print(f"[func entries] {tag}: worst |got - ref| / bound  " + "  ".join(f"{k} {worst[k]:.3g}" for k in fc.KINDS if k in worst))
    bad = [(what, kind, r) for what, kind, r in report if r["over"]]
    assert not bad, (tag, bad)


def expected_plan(f, what, n, assembled=False):
    """The one launch of a plain function (csrc/registry.h: plan_func) from the Python statement of FuncStage"""
    cls = f["meta"]["stage_class"]
    ld = f["NKKT"] | 1
    staged = what != CON and not assembled and cls > 0
    apw = cls if staged else 64
    slot = SLOT[what] + ("_ASM" if assembled else "")
    return [(slot, -(-n // apw), 1, 64, (2 + apw * ld) * 8 if staged else 0, 0, apw)], 0


# ---------------------------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("name", NAMES)
def test_every_function_every_kind(name):
    f = fc.load(name)
    mesh = Mesh(f, np.arange(f["x"].shape[0]))
    ev = evaluator(f, mesh)
    slots = fc.block_slots(ev.IR, ev.OR)
    report = []
    for what in (JAC_ADJGRAD_HESS, JAC, JAC_ADJGRAD, CON, CON_ADJGRAD):
        assert ev.launch_plan(what) == expected_plan(f, what, ev.nseg), what
        check_eval(ev, f, mesh, what, slots, report)
    ev.close()
    assert_report(name, report)


# ---------------------------------------------------------------------------------------------------------------- b
TILED = ["pathcon", "lgl_integral4_quad2", "control_spline4_2", "control_spline4_3", "control_spline4_4", "control_spline4_5",
         "lgl_mesh_spacing3"]


def copy_trip_size(apw, nkkt):
    """n <= 3 APW whose last group holds napp applications with napp NKKT an exact multiple of 8 x 64 elements (a whole number of trips
    of the copy-out loop); where no napp <= APW gives one, the napp whose count is the nearest above a multiple."""
    exact = [k for k in range(1, apw + 1) if (k * nkkt) % 512 == 0]
    k = exact[0] if exact else min(range(1, apw + 1), key=lambda k: ((k * nkkt) % 512, k))
    return apw + k if k < apw else apw


def tiled_sizes(f):
    cls = f["meta"]["stage_class"]
    apw = cls if cls > 0 else 64
    sizes = [1, apw - 1, apw, apw + 1, 2 * apw + 1]
    if cls > 0:                                            # (class 0 stores directly: no copy-out loop)
        sizes.append(copy_trip_size(apw, f["NKKT"]))
    return apw, list(dict.fromkeys(sizes))


@pytest.mark.parametrize("name", TILED)
def test_every_staging_class_at_its_edges_by_tiling(name):
    f = fc.load(name)
    cls = f["meta"]["stage_class"]
    apw, sizes = tiled_sizes(f)
    for i, n in enumerate(sizes):
        mesh = Mesh(f, tiling(n, f["x"].shape[0]))
        ev = evaluator(f, mesh)
        if i == 0:
            assert ev.launch_plan(JAC_ADJGRAD_HESS)[0][0][6] == apw       # the function's own APW, from its launch plan
        slots = fc.block_slots(ev.IR, ev.OR)
        report = []
        for what in ((JAC_ADJGRAD_HESS, JAC, CON_ADJGRAD) if i == 0 else (JAC_ADJGRAD_HESS,)):
            plan = ev.launch_plan(what)
            assert plan == expected_plan(f, what, n), (n, what, plan)
            assert plan[0][0][1] == -(-n // apw) and plan[0][0][4] == ((2 + apw * (f["NKKT"] | 1)) * 8 if cls > 0 else 0)
            check_eval(ev, f, mesh, what, slots, report)
        ev.close()
        assert_report(f"{name} class {cls} x{n}", report)
    CLASSES_LAUNCHED.setdefault(cls, []).append((name, sizes))


def test_copy_trip_sizes_are_what_they_are_for():
    """(no device) the last group of the extra size copies a whole number of trips of 8 x 64 elements where the class has such a group,
    else the count nearest above a multiple: 57 blocks of 9 entries are 513 elements, one past a whole trip"""
    for name in TILED:
        f = fc.load(name)
        if f["meta"]["stage_class"] == 0:
            continue
        apw, sizes = tiled_sizes(f)
        n = copy_trip_size(apw, f["NKKT"])
        napp = n - (n - 1) // apw * apw
        assert n in sizes
        assert 1 <= napp <= apw and n <= 3 * apw
        assert (napp * f["NKKT"]) % 512 == min((k * f["NKKT"]) % 512 for k in range(1, apw + 1)), name
    assert copy_trip_size(64, 9) == 64 + 57 and (57 * 9) % 512 == 1


# ---------------------------------------------------------------------------------------------------------------- c
class BundleMeshes:
    """The members' meshes behind ONE solver vector X (a bundle takes one): every member's variables behind its own offset; the
    multipliers stay one vector per member."""

    def __init__(self, names):
        self.f = [fc.load(n) for n in names]
        self.mesh, self.vindex, xs = [], [], []
        off = 0
        for k, f in enumerate(self.f):
            cls = f["meta"]["stage_class"]
            n = 1 if names[k] == fc.BUNDLE_MEMBERS[-1] else 2 * (cls if cls > 0 else 64) + 1
            m = Mesh(f, tiling(n, f["x"].shape[0], seed=5 + k), var_offset=3 + k, con_offset=1 + k % 3)
            self.mesh.append(m)
            self.vindex.append((m.vindex + off).astype(np.int32))
            xs.append(m.X)
            off += m.n_primal
        self.X, self.n_primal = np.concatenate(xs), off


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_bundles_are_held_to_the_fixture(order):
    import torch
    names = list(fc.BUNDLE_MEMBERS if order == "forward" else fc.BUNDLE_MEMBERS[::-1])
    bm = BundleMeshes(names)
    evs = [evaluator(f, m, vindex=v, n_primal=bm.n_primal) for f, m, v in zip(bm.f, bm.mesh, bm.vindex)]
    assert sorted({f["meta"]["stage_class"] for f in bm.f}) == [0, 4, 8, 16, 32, 64] and evs[names.index("pairwise")].nseg == 1
    bundle = FunctionBundle(evs)
    assert bundle.name == jit.ensure_bundle([e.device_name for e in evs])
    X, Ls = dev_tensor(bm.X), [dev_tensor(m.L) for m in bm.mesh]
    reports = [[] for _ in evs]
    for what in (JAC_ADJGRAD_HESS, JAC_ADJGRAD, CON):
        outs = [outputs(e, what) for e in evs]
        torch.cuda.synchronize()
        bundle.eval_device(what, X, Ls if what != CON else [None] * len(evs), [o[0] for o in outs], [o[1] for o in outs], [o[2] for o in outs])
        torch.cuda.synchronize()
        for e, f, m, o, rep in zip(evs, bm.f, bm.mesh, outs, reports):
            check_outputs(e, f, m.pi, what, o, fc.block_slots(e.IR, e.OR), rep)
    bundle.close()
    for n, e, rep in zip(names, evs, reports):
        assert_report(f"bundle ({order}) member {n} x{e.nseg}", rep)
        e.close()


# ---------------------------------------------------------------------------------------------------------------- d
def location_map(ev, mesh):
    """slot -> location of a mesh, as a solver's sparsity analysis numbers them: one location per distinct (row, column) of the KKT
    matrix -- Hessian entries between two variables, Jacobian entries between a constraint row and a variable.  -> (locs[n, NKKT],
    number of locations)"""
    rr, cc = reference_slot_order(ev.IR, ev.OR)
    col = mesh.vindex[:, cc].astype(np.int64)
    hess = rr < ev.IR
    row = np.where(hess[None, :], mesh.vindex[:, np.minimum(rr, ev.IR - 1)], mesh.n_primal + mesh.cindex[:, np.maximum(rr - ev.IR, 0)])
    lo, hi = np.minimum(row, col), np.maximum(row, col)
    _, inv = np.unique(hi.ravel() * (mesh.n_primal + mesh.n_equal) + lo.ravel(), return_inverse=True)
    return inv.reshape(col.shape).astype(np.int32), int(inv.max()) + 1


def assembled_own_locations(ev, f, mesh, tag):
    """Every slot a location of its own: the assembled kernels' entries held to the fixture.  -> the blocks of JAC_ADJGRAD_HESS"""
    import torch
    n, nk = ev.nseg, ev.NKKT
    hslot, jslot = fc.block_slots(ev.IR, ev.OR)
    rng = np.random.default_rng(3)
    perm = rng.permutation(n * nk).astype(np.int32).reshape(n, nk)        # (not the identity: the map is read, not assumed)
    ev.set_kkt_map(perm, n * nk)
    X, L = dev_tensor(mesh.X), dev_tensor(mesh.L)
    blocks = None
    for what in (JAC_ADJGRAD_HESS, JAC_ADJGRAD):
        assert ev.launch_plan(what, assembled=True) == expected_plan(f, what, n, assembled=True)
        prior = rng.uniform(-1, 1, n * nk)
        vals, fx, agx = dev_tensor(prior), nan_tensor(n * ev.OR), nan_tensor(n * ev.IR)
        torch.cuda.synchronize()
        ev.eval_assembled_device(what, X, L, fx, agx, vals)
        torch.cuda.synchronize()
        got = vals.cpu().numpy()[perm]
        report = [(KIND_NAMES[what], kind, fc.check(g, f, mesh.pi, kind))
                  for kind, g in (("fx", fx.cpu().numpy()), ("gx", agx.cpu().numpy()), ("jx", got[:, jslot.ravel()]))]
        if what == JAC_ADJGRAD_HESS:
            report.append((KIND_NAMES[what], "hx", fc.check(got[:, hslot], f, mesh.pi, "hx")))
            blocks = got
        else:
            assert np.array_equal(got[:, hslot], prior[perm][:, hslot]), "Hessian locations of a Jacobian kind keep their contents"
        assert_report(f"{tag} {SLOT[what]}_ASM x{n}", report)
    return blocks


@pytest.mark.parametrize("name", ["pathcon", "control_spline4_3", "control_spline4_5"])
def test_assembled_forms(name):
    """The tiled mesh shares every variable between many applications, so many blocks add into one Hessian location (three or more:
    the staged cells, summed in a fixed order): within 4 u sum |c| of the long-double scatter of the blocks just checked -- the value
    the array held before counted among the contributions, it is one --; every application keeps constraint rows of its own, as the
    constraints of a phase do, and the last one variables of its own: those locations take one contribution and are bit for bit
    prior + entry, or the entry itself under ``target_zeroed``; locations no slot names are unchanged."""
    f = fc.load(name)
    n = 2 * 64 + 1
    mesh = Mesh(f, tiling(n, f["x"].shape[0]), private_last=True, private_rows=True)
    ev = evaluator(f, mesh)
    blocks = assembled_own_locations(ev, f, mesh, name)
    locs, nloc = location_map(ev, mesh)
    pad = 7                                                 # locations of other constraints, before and after
    locs = locs + pad
    nvalues = nloc + 2 * pad
    ev.set_kkt_map(locs, nvalues)
    flat = locs.ravel()
    count = np.bincount(flat, minlength=nvalues)
    assert count.max() >= 3 and np.sum(count == 1) >= ev.NKKT and np.all(count[:pad] == 0) and np.all(count[-pad:] == 0)
    total = np.zeros(nvalues, dtype=np.longdouble)
    np.add.at(total, flat, blocks.ravel().astype(np.longdouble))
    mag = np.bincount(flat, weights=np.abs(blocks.ravel()), minlength=nvalues)
    prior = np.random.default_rng(4).uniform(-1, 1, nvalues)
    vals = prior.copy()
    ev.eval_assembled(JAC_ADJGRAD_HESS, mesh.X, mesh.L, vals)
    single, many = count == 1, count > 1
    want = prior + total.astype(np.float64)                 # (one contribution: the entry is a double, prior + entry one rounded sum)
    err = np.abs(vals - (prior.astype(np.longdouble) + total)).astype(np.float64)
    ratio = np.divide(err, 4.0 * fc.U * (mag + np.abs(prior)), out=np.zeros_like(err), where=mag > 0)
    print(f"[func entries] {name} assembled x{n}: {int(many.sum())} shared locations, up to {int(count.max())} contributions, worst "
          f"|assembled - scatter| / (4 u sum|c|) = {ratio[many].max():.3g}; {int(single.sum())} single locations, "
          f"{int(np.sum(vals[single] != want[single]))} of them not bit for bit")
    assert np.array_equal(vals[count == 0], prior[count == 0])
    assert np.array_equal(vals[single], want[single])
    assert np.all(err[many] <= 4.0 * fc.U * (mag[many] + np.abs(prior[many])))
    zeroed = np.zeros(nvalues)
    ev.eval_assembled(JAC_ADJGRAD_HESS, mesh.X, mesh.L, zeroed, target_zeroed=True)
    assert np.array_equal(zeroed[single], total[single].astype(np.float64)) and np.all(zeroed[count == 0] == 0.0)
    again = np.zeros(nvalues)                               # the many-way locations are summed in a fixed order: twice, bit for bit
    ev.eval_assembled(JAC_ADJGRAD_HESS, mesh.X, mesh.L, again, target_zeroed=True)
    assert np.array_equal(again, zeroed)
    assert np.all(np.abs(zeroed[many] - total[many]).astype(np.float64) <= 4.0 * fc.U * mag[many])
    ev.close()


def test_assembled_objective_shaped_map_drops_the_jacobian():
    """lgl_integral4_wide7 as an integral objective is assembled: its Jacobian slots are -1 in the map (an objective has no row), the
    would-be locations stay untouched and the Hessian entries land."""
    import torch
    f = fc.load("lgl_integral4_wide7")
    n = 2 * 8 + 1
    mesh = Mesh(f, tiling(n, f["x"].shape[0]))
    ev = evaluator(f, mesh)
    hslot, jslot = fc.block_slots(ev.IR, ev.OR)
    own = np.arange(n * ev.NKKT, dtype=np.int32).reshape(n, ev.NKKT)
    dropped = own.copy()
    dropped[:, jslot.ravel()] = -1
    ev.set_kkt_map(dropped, n * ev.NKKT)
    assert ev.launch_plan(JAC_ADJGRAD_HESS, assembled=True) == expected_plan(f, JAC_ADJGRAD_HESS, n, assembled=True)
    prior = np.random.default_rng(6).uniform(-1, 1, n * ev.NKKT)
    vals, fx, agx = dev_tensor(prior), nan_tensor(n * ev.OR), nan_tensor(n * ev.IR)
    torch.cuda.synchronize()
    ev.eval_assembled_device(JAC_ADJGRAD_HESS, dev_tensor(mesh.X), dev_tensor(mesh.L), fx, agx, vals)
    torch.cuda.synchronize()
    got = vals.cpu().numpy()[own]
    assert np.array_equal(got[:, jslot.ravel()], prior[own][:, jslot.ravel()])
    report = [("JAC_ADJGRAD_HESS", kind, fc.check(g, f, mesh.pi, kind))
              for kind, g in (("fx", fx.cpu().numpy()), ("gx", agx.cpu().numpy()), ("hx", got[:, hslot]))]
    ev.close()
    assert_report(f"lgl_integral4_wide7 K_FUNC2_ASM, Jacobian dropped, x{n}", report)


def test_all_six_staging_classes_were_launched():
    """(after test b) which function ran which class at which sizes"""
    for cls in (64, 32, 16, 8, 4, 0):
        print(f"[func entries] staging class {cls}: " + "; ".join(f"{n} x{s}" for n, s in CLASSES_LAUNCHED.get(cls, [])))
    assert set(CLASSES_LAUNCHED) == {64, 32, 16, 8, 4, 0}, sorted(CLASSES_LAUNCHED)
