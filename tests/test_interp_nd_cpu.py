"""``vf.InterpTable2D`` / ``vf.InterpTable3D`` on the host (the reference's InterpTable2D / InterpFunction2D and InterpTable3D /
InterpFunction3D): the interpolant with its gradient and Hessian against the 50-digit fixture tests/golden/interp_nd/tables.npz,
entry by entry within the fixture's bounds, through the host objects, through ``ir.evaluate`` of the symbolic derivatives and through
the plain-C printer compiled here; exactness on polynomial data; constructors, look-up and errors; what a module embeds; the cap.

Measured here (worst |got - ref| / bound over every entry of the four tables): see the prints of each test; the float64 restatement
of tests/interp_nd_checker.py uses at most 0.21 of a bound (QUARTER asks for 0.25)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import warnings

import numpy as np
import pytest

import interp_nd_cases as cases
import interp_nd_checker as ck
from asset_asrl_amd import vf
from asset_asrl_amd.vf import codegen
from asset_asrl_amd.vf.codegen import differentiate_function, emit_c, emit_hip_functor
from asset_asrl_amd.vf.ir import evaluate
from helpers import rel_err

HERE = os.path.dirname(os.path.abspath(__file__))


def _check_table(name, v, g, H, what):
    e = ck.entries(name)
    worst = max(ck.check(v, *e["v"], f"{what} {name} value"), ck.check(g, *e["g"], f"{what} {name} gradient"),
                ck.check(H, *e["H"], f"{what} {name} Hessian"))
    print(f"{what} {name}: worst |got - ref| / bound = {worst:.3g}")
    return worst


def test_the_restatement_keeps_a_quarter_of_every_bound():
    used = ck.check_quarter()
    print("float64 restatement, share of the bound:", used)
    assert max(used.values()) <= ck.QUARTER


@pytest.mark.parametrize("name", ck.TABLES)
def test_host_interpolation_matches_the_fixture(name):
    tab, P = cases.table(name), ck.load()[f"{name}_P"]
    out = [tab.interp_deriv2(*p) for p in P]
    _check_table(name, [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], "host interp_deriv2")
    e = ck.entries(name)
    ck.check([tab.interp(*p) for p in P], *e["v"], f"{name} interp")
    d1 = [tab.interp_deriv1(*p) for p in P]
    ck.check([o[0] for o in d1], *e["v"], f"{name} interp_deriv1 value")
    ck.check([o[1] for o in d1], *e["g"], f"{name} interp_deriv1 gradient")
    M = tab.interp(*[P[:6, a].reshape(2, 3) for a in range(ck.DIM[name])])            # elementwise, as the reference's matrix overload
    assert M.shape == (2, 3) and np.array_equal(M.ravel(), [tab.interp(*p) for p in P[:6]])
    assert tab(*P[3]) == tab.interp(*P[3])                                             # numbers in, numbers out


def _symbolic_blocks(d, p):
    N = d.nin
    v = evaluate(d.f, p)[0]
    g = np.array(evaluate(list(d.J[0]), p))
    H = np.array(evaluate([d.H[max(i, j)][min(i, j)] for i in range(N) for j in range(N)], p, [1.0])).reshape(N, N)
    return v, g, H


@pytest.mark.parametrize("name", ck.TABLES)
def test_symbolic_derivatives_match_the_fixture_through_ir_evaluate(name):
    d = differentiate_function("interpnd_" + name, cases.table(name).vf())
    out = [_symbolic_blocks(d, p) for p in ck.load()[f"{name}_P"]]
    _check_table(name, [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], "ir.evaluate")
    ag = [evaluate(d.g, p, [1.0]) for p in ck.load()[f"{name}_P"]]                     # the adjoint gradient (a reverse sweep) with lam = 1
    ck.check(ag, *ck.entries(name)["g"], f"ir.evaluate {name} adjoint gradient")


@pytest.mark.parametrize("name", ck.TABLES)
def test_plain_c_build_matches_the_fixture(name, tmp_path):
    d = differentiate_function("interpnd_" + name, cases.function(name))
    text = emit_c(d, "tab")
    assert "static const double tab_TAB_" in text and "tab_tab_find(tab_TAB_" in text and "tab_tab_even(" in text
    (tmp_path / "tab.c").write_text(text)
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", str(tmp_path / "tab.c"), "-o", str(tmp_path / "tab.so"), "-lm"])
    L = C.CDLL(str(tmp_path / "tab.so"))
    N = ck.DIM[name]
    vs, gs, Hs, ags = [], [], [], []
    lam = np.ones(1)
    for p in ck.load()[f"{name}_P"]:
        y, f, J, g, H = np.array(p, dtype=float), np.zeros(1), np.zeros((1, N)), np.zeros(N), np.zeros((N, N))
        L.tab_fjgh(*[C.c_void_p(a.ctypes.data) for a in (y, lam, f, J, g, H)])
        f1, J1 = np.zeros(1), np.zeros((1, N))
        L.tab_fj(*[C.c_void_p(a.ctypes.data) for a in (y, f1, J1)])
        assert np.array_equal(f1, f) and np.array_equal(J1, J)
        vs.append(f[0]), gs.append(J[0]), Hs.append(H), ags.append(g)
    _check_table(name, vs, gs, Hs, "plain C")
    ck.check(ags, *ck.entries(name)["g"], f"plain C {name} adjoint gradient")


# ---- exactness on polynomial data
def _exactness_points(name, rng, m=40):
    axes = cases.GRID[name]
    P = [[rng.uniform(a[0] - 0.3 * (a[1] - a[0]), a[-1] + 0.3 * (a[-1] - a[-2])) for a in axes] for _ in range(m)]
    P += [[a[0] - 0.3 * (a[1] - a[0]) for a in axes], [a[-1] + 0.3 * (a[-1] - a[-2]) for a in axes], [a[2] for a in axes]]
    return np.array(P)


@pytest.mark.parametrize("name", sorted(cases.POLY))
def test_a_table_of_polynomial_data_reproduces_the_polynomial(name):
    """cubic: degree <= 3 per variable; linear: degree <= 1 per variable -- value, gradient and Hessian, inside the grid and up to 0.3
    of an end cell outside it.  rel_err < 1e-12 (two float64 forms of one function: tests/test_gpu_jit.py,
    test_composed_user_ode_block_form_against_flat_form), held here to a quarter of that."""
    tab = cases.poly_table(name)
    worst = 0.0
    for p in _exactness_points(name, np.random.default_rng(7)):
        got, ref = tab.interp_deriv2(*p), cases.poly_blocks(name, p)
        worst = max([worst] + [rel_err(a, b) for a, b in zip(got, ref)])
    print(f"{name}: worst rel_err against the polynomial {worst:.3g}")
    assert worst < 0.25 * 1e-12
    if name.startswith("cubic"):                                       # the nodal derivatives are the polynomial's own
        d = len(cases.GRID[name])
        node = [a[1] for a in cases.GRID[name]]
        mixed = cases.poly_np(name, node, [1] * d)
        stored = tab._Q[(1 << d) - 1][(1, 1) if d == 2 else (1, 1, 1)]
        assert abs(stored - mixed) < 1e-12 * max(1.0, abs(mixed))


def test_the_table_ode_and_its_polynomial_twin_agree_through_the_plain_c_builds(tmp_path):
    """The pair of tests/test_gpu_interp_nd.py's phase test, on the CPU first: f, J, g, H of the table ODE and of its twin at states
    past the table ends sit below a quarter of rel_err < 1e-12."""
    libs = []
    for twin in (False, True):
        d = cases.make_ode(twin).derivatives()
        src = tmp_path / f"ode{int(twin)}.c"
        src.write_text(emit_c(d, "ode"))
        subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", str(src), "-o", str(tmp_path / f"ode{int(twin)}.so"), "-lm"])
        libs.append(C.CDLL(str(tmp_path / f"ode{int(twin)}.so")))
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(200):
        y = np.array([rng.uniform(-1.9, 1.9), rng.uniform(-1.8, 1.8), rng.uniform(-0.7, 2.8), rng.uniform(-1.7, 1.7)])
        lam = rng.uniform(-1, 1, 2)
        out = []
        for L in libs:
            f, J, g, H = np.zeros(2), np.zeros((2, 4)), np.zeros(4), np.zeros((4, 4))
            L.ode_fjgh(*[C.c_void_p(a.ctypes.data) for a in (y, lam, f, J, g, H)])
            out.append((f, J, g, H))
        worst = max([worst] + [rel_err(a, b) for a, b in zip(*out)])
        assert np.array_equal(out[0][3], out[0][3].T)
    print(f"table ODE against its twin: worst rel_err {worst:.3g}")
    assert worst < 0.25 * 1e-12


# ---- constructors, look-up, errors
def test_constructors_checks_and_lookup():
    xs, ys, zs = np.linspace(0.0, 2.0, 6), np.array([0.0, 0.3, 0.5, 1.0, 1.2, 1.7, 2.0]), np.linspace(-1.0, 1.0, 5)
    Z = np.add.outer(np.cos(ys), np.sin(xs))                           # Zs[iy, ix]
    F = np.sin(xs)[:, None, None] + np.cos(ys)[None, :, None] * zs[None, None, :]
    t2 = vf.InterpTable2D(xs, ys, Z)
    assert (t2.kind, t2.xeven, t2.yeven) == ("cubic", True, False)
    assert vf.InterpTable2D(xs, ys, Z, kind="Cubic").digest == t2.digest and vf.InterpTable2D(xs, ys, Z, "Linear").kind == "linear"
    t3 = vf.InterpTable3D(xs, ys, zs, F, kind="cubic", cache=True)     # (cache: accepted and ignored)
    assert (t3.xeven, t3.yeven, t3.zeven) == (True, False, True) and vf.InterpTable3D(xs, ys, zs, F).digest == t3.digest
    assert vf.InterpTable3D(xs, ys, zs, F, "linear").digest != t3.digest
    assert not hasattr(vf, "InterpTable4D")
    for args, msg in (((xs, ys, Z, "quintic"), "Unrecognized interpolation type"), ((xs[:4], ys, Z[:, :4]), "X coordinates must be larger than 4"),
                      ((xs, ys[:4], Z[:4]), "Y  coordinates must be larger than 4"), ((xs, ys, Z[:, :5]), "X coordinates must match cols in Z matrix"),
                      ((xs, ys, Z[:6]), "Y coordinates must match rows in Z matrix"), ((xs[::-1].copy(), ys, Z), "X Coordinates must be in ascending order"),
                      ((xs, ys[::-1].copy(), Z), "Y Coordinates must be in ascending order")):
        with pytest.raises(ValueError, match=msg):
            vf.InterpTable2D(*args)
    for args, msg in (((xs, ys, zs, F, "quintic"), "Unrecognized interpolation type"), ((xs[:4], ys, zs, F[:4]), "X coordinates must be larger than 4"),
                      ((xs, ys[:4], zs, F[:, :4]), "Y  coordinates must be larger than 4"), ((xs, ys, zs[:4], F[:, :, :4]), "Z  coordinates must be larger than 4"),
                      ((xs, ys, zs, F[:5]), "X coordinates must be first dimension of value tensor"),
                      ((xs, ys, zs, F[:, :6]), "Y coordinates must be second dimension of value tensor"),
                      ((xs, ys, zs, F[:, :, :4].repeat(2, axis=2)[:, :, :6]), "Z coordinates must be third dimension of value tensor"),
                      ((xs[::-1].copy(), ys, zs, F), "X coordinates must be in ascending order"),
                      ((xs, ys[::-1].copy(), zs, F), "Y coordinates must be in ascending order"),
                      ((xs, ys, zs[::-1].copy(), F), "Z coordinates must be in ascending order")):
        with pytest.raises(ValueError, match=msg):
            vf.InterpTable3D(*args)
    # evenly spaced or not, per axis: the largest deviation from linspace against 1e-12 |total|, just under and just over
    for bump, even in ((0.9e-12, True), (1.1e-12, False)):
        x2 = xs.copy()
        x2[2] += bump * 2.0
        assert vf.InterpTable2D(x2, ys, Z).xeven is even and vf.InterpTable2D(ys, x2, Z.T.copy()).yeven is even
        assert vf.InterpTable3D(ys, ys, x2, np.zeros((7, 7, 6))).zeven is even
    # the element: by division / bisection, clamped; extrapolation from the end cell
    assert t2._elems((0.41, 1.1)) == [1, 3] and t2._elems((-5.0, 9.0)) == [0, 5] and t2._elems((2.0, 2.0)) == [4, 5]
    assert t2.find_elem(ys, 1.1) == 3 and t2.find_elem(ys, -1.0) == -1 and t2.find_elem(ys, 5.0) == 6        # (not clamped: InterpTable2D.h:202-208)
    assert vf.InterpTable3D.find_elem(ys, False, 5.0) == 5 and vf.InterpTable3D.find_elem(xs, True, 0.41) == 1 and t3.find_elem(xs, True, -3.0) == 0
    # outside the data: a warning per axis, or an error when asked for
    with pytest.warns(UserWarning, match="y coordinate falls outside of InterpTable2D range"):
        t2.interp(1.0, 2.5)
    with pytest.warns(UserWarning, match="z coordinate falls outside of InterpTable3D range"):
        t3.interp_deriv1(1.0, 1.0, -1.5)
    t2.ThrowOutOfBounds = True
    with pytest.raises(ValueError, match="x coordinate"):
        t2.interp(-0.5, 1.0)
    t2.WarnOutOfBounds = t2.ThrowOutOfBounds = False
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        t2.interp(-0.5, 2.5), t2.interp(0.5, 1.5)
    # scalar and array arguments
    A = t2.interp(np.array([[0.1, 0.2], [0.3, 0.4]]), np.array([[1.0, 1.1], [1.2, 1.3]]))
    assert A.shape == (2, 2) and A[1, 0] == t2.interp(0.3, 1.2) and isinstance(t2.interp(0.3, 1.2), float)
    v, g, H = t3.interp_deriv2(0.3, 1.2, 0.1)
    assert np.shape(g) == (3,) and np.shape(H) == (3, 3) and np.array_equal(H, H.T)
    vl, gl, Hl = vf.InterpTable3D(xs, ys, zs, F, "linear").interp_deriv2(0.3, 1.2, 0.1)
    assert np.all(np.diag(Hl) == 0.0) and Hl[1, 2] != 0.0                              # a multilinear cell: the cross terms only


def test_expression_forms_share_their_nodes_and_constants_fold():
    t2, t3 = cases.table("c2"), cases.table("c3")
    a2, a3 = vf.Arguments(2), vf.Arguments(3)
    assert t2(a2[0], a2[1]).outs[0] is t2(a2).outs[0] is t2.sf().outs[0] is t2.vf().outs[0]
    assert t3(a3[0], a3[1], a3[2]).outs[0] is t3(a3).outs[0] is t3.sf().outs[0] is t3.vf().outs[0]
    assert (t2.sf().IRows(), t2.sf().ORows(), t3.vf().IRows(), t3.vf().ORows()) == (2, 1, 3, 1)
    a5 = vf.Arguments(5)
    f = t3(a5[4] * 0.5, a5[1], a5.head(3)[2])
    assert (f.IRows(), f.ORows()) == (5, 1)
    assert abs(evaluate(f.outs, [0, 0.7, 0.2, 0, 0.4])[0] - t3.interp(0.2, 0.7, 0.2)) < 1e-15
    for bad in (lambda: t2(a3), lambda: t3(a2), lambda: t2(a2[0], a3[1]), lambda: t2(a2[0]), lambda: t3(a3[0], a3[1]), lambda: t2(a2, a2[0])):
        with pytest.raises(ValueError):
            bad()
    # constant arguments fold to constants: no table node is left, the number is the host's
    c = t2(vf.ConstantScalar(3, 0.3), vf.ConstantScalar(3, 1.1))
    assert c.outs[0].is_const() and c.outs[0].value == t2.interp(0.3, 1.1)
    c3 = cases.table("l3")(vf.ConstantScalar(1, 0.3), vf.ConstantScalar(1, 0.4), vf.ConstantScalar(1, 0.1))
    assert c3.outs[0].is_const() and c3.outs[0].value == cases.table("l3").interp(0.3, 0.4, 0.1)


# ---- what a module embeds
def test_equal_tables_are_emitted_once_and_a_changed_table_is_another_module():
    fx = ck.load()
    axes, data = ck.axes_of("c2"), fx["c2_data"]
    ta, tb = vf.InterpTable2D(*axes, data), vf.InterpTable2D(*[a.copy() for a in axes], data.copy())
    assert ta.digest == tb.digest == cases.table("c2").digest
    a = vf.Arguments(2)
    d = differentiate_function("twice", vf.stack([ta(a[0], a[1]), tb(a[1] * 0.5, a[0] + 1.0)]))
    hip = emit_hip_functor(d, "Twice")
    assert hip.count(f"static constexpr double TAB_{ta.digest}_r[") == 1 and hip.count("static constexpr double TAB_") == 3   # the data, two axes
    assert f"asset_tab_find(TAB_{ta._axes[1].digest}_t, 7," in hip and "asset_tab_even(" in hip     # bisection on the uneven axis, division on the even one
    bodies = [b for b in hip.split("__host__ __device__ static")[1:] if "asset_tab_" in b]
    assert any(" void fjgh(" in b for b in bodies)
    for b in bodies:                                                   # in every body (f; f + J; f + J + g + H; ...): one look-up per axis per
        assert b.count("asset_tab_find(") + b.count("asset_tab_even(") == 4, b[:80]     # table use, shared by all levels of that body
    changed = data.copy()
    changed[2, 3] += 1e-9
    tc = vf.InterpTable2D(*axes, changed)
    assert tc.digest != ta.digest
    assert emit_hip_functor(differentiate_function("one", tc.vf()), "F") != emit_hip_functor(differentiate_function("one", ta.vf()), "F")
    # the two layouts of a cubic table are two arrays and two bodies
    old = vf.functions.TABLE_LAYOUT
    try:
        vf.functions.TABLE_LAYOUT = "planes"
        planes = emit_hip_functor(differentiate_function("one", ta.vf()), "F")
    finally:
        vf.functions.TABLE_LAYOUT = old
    assert f"TAB_{ta.digest}_p[" in planes and f"TAB_{ta.digest}_r[" not in planes


def test_generated_source_of_every_existing_ode_and_function_is_unchanged():
    """sha256 of ``emit_hip_functor`` for every ODE of tests/helpers.py and every function of tests/vf_cases.py, recorded on the commit
    before the tables over several axes: the table nodes were generalised to named arrays, and no existing module may move."""
    import helpers
    import vf_cases
    with open(os.path.join(HERE, "golden", "interp_nd", "source_digests.json")) as fh:
        want = json.load(fh)
    odes = [("vanderpol", helpers.make_vanderpol), ("coupled12", lambda: helpers.make_coupled(12)), ("coupled16", lambda: helpers.make_coupled(16)),
            ("driven14", lambda: helpers.make_driven(14)), ("driven20", lambda: helpers.make_driven(20)), ("manyparams", helpers.make_manyparams),
            ("nested_orbit", helpers.make_nested_orbit), ("nested_orbit_flat", lambda: helpers.make_nested_orbit(True)),
            ("switched", helpers.make_switched), ("guarded", helpers.make_guarded), ("tabulated", helpers.make_tabulated)]
    odes += [("shape_%d_%d_%d" % s, (lambda s=s: helpers.make_shape(*s))) for s in helpers.SHAPES]
    got = {"ode:" + name: hashlib.sha256(emit_hip_functor(mk().derivatives(), "OdeUser").encode()).hexdigest() for name, mk in odes}
    for name, flat in vf_cases.DEVICE_FORMS:
        d = vf_cases.build_flat(name)[1] if flat else differentiate_function(name, vf_cases.build(name))
        got["fn:" + vf_cases.device_name(name, flat)] = hashlib.sha256(emit_hip_functor(d, "FnUser").encode()).hexdigest()
    assert got == want


def test_the_cap_on_embedded_table_data():
    n = int(np.sqrt(0.6 * codegen.TABLE_ENTRY_CAP))
    xs = np.linspace(0.0, 1.0, n)
    big = vf.InterpTable2D(xs, xs, np.add.outer(xs, xs * xs), kind="linear")           # (linear tables: quick to construct, one number per node)
    assert big.entries <= codegen.TABLE_ENTRY_CAP
    assert f"TAB_{big.digest}_r[{n * n}]" in emit_c(differentiate_function("under", big.vf()), "under")
    m = 1 + int(np.ceil(codegen.TABLE_ENTRY_CAP ** 0.5))
    ys = np.linspace(0.0, 1.0, m)
    over = vf.InterpTable2D(ys, ys, np.add.outer(ys, ys * ys), kind="linear")
    over.WarnOutOfBounds = False
    assert over.entries > codegen.TABLE_ENTRY_CAP
    d = differentiate_function("over", over.vf())                                      # building and differentiating the expression is not capped
    for emit in (lambda: emit_hip_functor(d, "Over"), lambda: emit_c(d, "over")):
        with pytest.raises(ValueError, match="numbers of tabulated data in one module; the cap is"):
            emit()
    assert abs(over.interp(0.3, 0.6) - (0.6 + 0.09)) < 1e-6                            # the host interpolation is not
    # two tables under the cap each, over it together
    other = vf.InterpTable2D(xs, xs, np.add.outer(xs * xs, xs), kind="linear")
    a = vf.Arguments(2)
    both = differentiate_function("both", vf.stack([big(a[0], a[1]), other(a[0], a[1])]))
    assert big.entries + other.entries > codegen.TABLE_ENTRY_CAP > other.entries
    with pytest.raises(ValueError, match="the cap is"):
        emit_hip_functor(both, "Both")
