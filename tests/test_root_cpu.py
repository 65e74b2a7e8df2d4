"""``vf.ScalarRootFinder`` and ``astro.KeplerPropagator`` on the host: the implicit-function rules of vf/ir.py walked by ``ir.evaluate``
and the plain-C printer compiled with gcc, against the 50-digit fixture tests/golden/root/root.npz (differentiated Newton iteration,
another route; bounds per entry: tests/golden/make_golden_root.py); the iteration's semantics, compared exactly with a restatement; the
printed text; the argument checks; the propagator against the propagation fixture; the run-time modules, compile-only; the twin pair.

Measured here (worst |got - ref| / bound): ir.evaluate and plain C alike 0.34 (kepler_eq), 0.24 (cubic), 0.74 (given_step), 0.66 (composed),
0.32 (twice), 0.33 (kepler_prop); inside the parabolic band 0.33; the twin pair 3.9e-16 in rel_err."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import controller_cases
import event_cases
import root_cases as cases
from asset_asrl_amd import astro, jit, vf
from asset_asrl_amd.vf import codegen
from asset_asrl_amd.vf.codegen import differentiate_function, emit_c, emit_hip_functor
from asset_asrl_amd.vf.ir import ROOTS, count_ops, evaluate
from helpers import rel_err

U = cases.U


def _check(name, f, J, H, what):
    """f [m, n], J [m, n, N], H [m, N, N] (lam^T H for the fixture's lam) within the stored bounds; the guess's row and column exactly 0"""
    worst = max(cases.close(f, *cases.entries(name, "f"), f"{what} {name} value"),
                cases.close(J, *cases.entries(name, "J"), f"{what} {name} Jacobian"),
                cases.close(H, *cases.entries(name, "H"), f"{what} {name} adjoint Hessian"))
    if cases.HAS_GUESS[name]:
        J, H = np.asarray(J), np.asarray(H)
        assert not J[:, :, 0].any() and not H[:, 0, :].any() and not H[:, :, 0].any()
    print(f"{what} {name}: worst |got - ref| / bound = {worst:.3g}")


# ---- 1. the symbolic rules
@pytest.mark.parametrize("name", cases.CASES)
def test_symbolic_rules_match_the_fixture_through_ir_evaluate(name):
    fn = cases.function(name)
    N, n = cases.SIZES[name]
    d = differentiate_function(name, fn)
    fx = cases.load()
    low = [d.H[max(i, j)][min(i, j)] for i in range(N) for j in range(N)]
    f, J, H = [], [], []
    for p, lam in zip(fx[f"{name}_P"], fx[f"{name}_lam"]):
        f.append(fn.compute(p))
        J.append(np.array(evaluate([e for r in d.J for e in r], p)).reshape(n, N))
        H.append(np.array(evaluate(low, p, lam)).reshape(N, N))
    _check(name, f, J, H, "ir.evaluate")
    if cases.HAS_GUESS[name]:                                          # ... and structurally: no expression at all
        assert all(d.J[k][0] is vf.functions.G.zero for k in range(n)) and all(d.H[i][0] is vf.functions.G.zero for i in range(N))


# ---- 2. the plain-C printer
@pytest.mark.parametrize("name", cases.CASES)
def test_emitted_c_matches_the_fixture(name, tmp_path):
    N, n = cases.SIZES[name]
    d = differentiate_function(name, cases.function(name))
    text = emit_c(d, "rt")
    assert "for (int " in text and "break;" in text and "#pragma" not in text
    (tmp_path / "rt.c").write_text(text)
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", str(tmp_path / "rt.c"), "-o", str(tmp_path / "rt.so"), "-lm"])
    L = C.CDLL(str(tmp_path / "rt.so"))
    fx = cases.load()
    fs, Js, Hs, f0s = [], [], [], []
    for p, lam in zip(fx[f"{name}_P"], fx[f"{name}_lam"]):
        y, lam = np.array(p, dtype=float), np.array(lam, dtype=float)
        f, J, g, H = np.zeros(n), np.zeros((n, N)), np.zeros(N), np.zeros((N, N))
        L.rt_fjgh(*[C.c_void_p(a.ctypes.data) for a in (y, lam, f, J, g, H)])
        f1, J1, f0 = np.zeros(n), np.zeros((n, N)), np.zeros(n)
        L.rt_fj(*[C.c_void_p(a.ctypes.data) for a in (y, f1, J1)])
        L.rt_f(*[C.c_void_p(a.ctypes.data) for a in (y, f0)])
        assert np.array_equal(f1, f) and np.array_equal(J1, J)
        assert rel_err(g, J.T @ lam) < 1e-13 and np.array_equal(H, H.T)
        fs.append(f), Js.append(J), Hs.append(H), f0s.append(f0)
    _check(name, fs, Js, Hs, "plain C")
    cases.close(f0s, *cases.entries(name, "f"), f"plain C {name} value body")       # (its own lowered quotients: not bitwise the level-2 body's)


def test_the_propagator_inside_the_parabolic_band():
    """|psi| < conictol: the constants 1/2 and 1/6 stand for the Stumpff functions; within twice the 50-digit difference the two make."""
    fx = cases.load()
    kp = cases.function("kepler_prop")
    got = np.array([kp.compute(p) for p in fx["kepler_prop_band_P"]])
    worst = cases.close(got, fx["kepler_prop_band_f"].astype(np.longdouble), fx["kepler_prop_band_fB"], "band")
    print(f"band: worst share {worst:.3g}")


# ---- 3. the iteration, exactly
def _newton(F, D, s, p, iters, tol):
    for _ in range(iters):
        r = F(s, *p)
        if abs(r) < tol:
            break
        s -= r / D(s, *p)
    return s


def test_iteration_semantics_exactly():
    F = lambda E, e, M: E - e * math.sin(E) - M                        # noqa: E731
    D = lambda E, e, M: 1.0 - e * math.cos(E)                          # noqa: E731
    y = [0.7, 0.8, 0.9]
    assert cases.kepler_equation(0).compute(y)[0] == 0.7                                            # iters = 0: the guess
    assert cases.kepler_equation(1).compute(y)[0] == 0.7 - F(*y) / D(*y)                            # one Newton step
    assert cases.kepler_equation(10, tol=abs(F(*y)) * 1.5).compute(y)[0] == 0.7                     # |F(guess)| < tol: the guess
    for k in (2, 3, 10):
        assert cases.kepler_equation(k).compute(y)[0] == _newton(F, D, 0.7, y[1:], k, cases.TOL)
    Fc = lambda s, a, b: s ** 3 + a * s - b                            # noqa: E731
    Dg = lambda s, a, b: 3.0 * (s * s) + a + 0.1                       # noqa: E731
    yc = [0.0, 0.6, 1.7]
    for k in (1, 4, 60):                                               # the given form steps with dfx
        assert cases.cubic_equation(k, given=True).compute(yc)[0] == _newton(Fc, Dg, 0.0, yc[1:], k, cases.TOL)
    Dc = lambda s, a, b: 3.0 * (s * s) + a                             # noqa: E731
    assert cases.cubic_equation(4, given=True).compute(yc)[0] != cases.cubic_equation(4).compute(yc)[0] == _newton(Fc, Dc, 0.0, yc[1:], 4, cases.TOL)
    far = [40.0, 0.6, 1.7]                                             # not converged after 3 passes: the last iterate, nothing raised
    got = cases.cubic_equation(3).compute(far)[0]
    assert got == _newton(Fc, Dc, 40.0, far[1:], 3, cases.TOL) and abs(Fc(got, *far[1:])) > 1.0
    # the derivative of the given form is the residual's, not the step's: ds/db = 1 / (3 s^2 + a)
    d = differentiate_function("g", cases.cubic_equation(60, given=True))
    s = cases.cubic_equation(60, given=True).compute(yc)[0]
    assert abs(evaluate([d.J[0][2]], yc)[0] - 1.0 / Dc(s, *yc[1:])) < 1e-15


# ---- 4. the printed text
def _bodies(text):
    out = {}
    for b in text.split("__host__ __device__ static")[1:]:
        out[b.split("void ")[1].split("(")[0]] = b
    return out


def test_printed_text_one_loop_per_root():
    tw = _bodies(emit_hip_functor(differentiate_function("twice", cases.function("twice")), "Tw"))
    assert tw["fjgh"].count("for (int ") == 2 and tw["fjgh"].count("#pragma unroll 1") == 2 and tw["fjgh"].count("break;") == 2
    d = cases.make_ode(False).derivatives()
    text = emit_hip_functor(d, "Od")
    b = _bodies(text)
    for name in ("f", "fj", "fjgh", "f_save", "fj_save"):
        assert b[name].count("for (int ") == 1, name
    assert "NSAVE = 2" in text                                         # sin t and the root
    assert b["fjgh_load"].count("for (int ") == 0 and "in.saved(" in b["fjgh_load"]     # the derivative pass does not iterate again
    assert "sqrt(" not in text and "for (int " not in emit_hip_functor(cases.make_ode(True).derivatives(), "Tw")
    # operation counts: iters x the template (an upper bound)
    k10 = cases.kepler_equation(10)
    tpl = ROOTS[k10.outs[0].value]
    assert tpl.iters == 10 and count_ops([tpl.F]) >= 4
    assert differentiate_function("k", k10).stats()["ops_f"] >= 10 * count_ops([tpl.F, tpl.D])
    # content keys: the same equation built twice is the same node and the same text; another tolerance is another
    assert cases.kepler_equation(10).outs[0] is k10.outs[0] and cases.kepler_equation(10, 1e-13).outs[0] is not k10.outs[0]
    assert cases.kepler_equation(10).outs[0].skey == k10.outs[0].skey != cases.kepler_equation(11).outs[0].skey


# ---- 5. argument errors
def test_argument_errors():
    a3, a2 = vf.Arguments(3), vf.Arguments(2)
    fx = a3[0] * a3[0] - a3[1] + a3[2]
    cases_ = [
        (lambda: vf.ScalarRootFinder(a3, 10, 1e-12), "fx is not a scalar function"),
        (lambda: vf.ScalarRootFinder(fx, a3, 10, 1e-12), "dfx is not a scalar function"),
        (lambda: vf.ScalarRootFinder(fx, a2[0] * 2.0, 10, 1e-12), r"dfx has 2 inputs \(IRows\), fx has 3"),
        (lambda: vf.ScalarRootFinder(fx, -1, 1e-12), "iters = -1 is not a non-negative integer"),
        (lambda: vf.ScalarRootFinder(fx, 10, 0.0), "tol = 0.0 is not a finite positive number"),
        (lambda: vf.ScalarRootFinder(fx, 10, -1e-9), "is not a finite positive number"),
        (lambda: vf.ScalarRootFinder(fx, 10, float("inf")), "is not a finite positive number"),
        (lambda: vf.ScalarRootFinder(fx, 10, float("nan")), "is not a finite positive number"),
    ]
    inner = vf.ScalarRootFinder(fx, 10, 1e-12)
    nested = inner.eval(vf.stack([a3[0], a3[1], a3[2]])) + a3[0] * a3[0]
    cases_.append((lambda: vf.ScalarRootFinder(nested, 10, 1e-12), "the template of a root holds another root"))
    cases_.append((lambda: vf.ScalarRootFinder(fx, nested, 10, 1e-12), "the template of a root holds another root"))
    for call, msg in cases_:
        with pytest.raises(ValueError, match=msg):
            call()
    with pytest.raises(ValueError, match="mu = "):
        astro.KeplerPropagator(-1.0)
    # a root as a PARAMETER of another is fine
    outer = vf.ScalarRootFinder(fx, 10, 1e-12).eval(vf.stack([a3[0], inner, a3[2]]))
    assert outer.IRows() == 3 and np.isfinite(outer.compute([1.0, 2.0, 0.5])[0])


# ---- 6. the propagator
def test_kepler_propagator_against_the_propagation_fixture():
    """The three Kepler arcs of tests/golden/propagate/propagate.npz are points 0..2 of the ``kepler_prop`` case (the generator asserts that
    its 50-digit values are that file's x_exact, S_exact[:, :6] and dtf_exact, which it stores rounded to float64): value, d/d[R, V] and
    d/d dt against that file, within the case's bounds plus that rounding."""
    import propagate_checker as pck
    fx, own = pck.fixture()[1], cases.load()
    dflt = astro.KeplerPropagator(1.0)                                 # the reference's defaults (KeplerPropagator.h:291-293)
    tpl = [ROOTS[n.value] for n in codegen.topo_order(dflt.outs) if n.op == "root"]
    assert (dflt.IRows(), dflt.ORows()) == (7, 6) and len(tpl) == 1 and (tpl[0].iters, tpl[0].tol, tpl[0].given) == (19, 1e-12, True)
    kp = cases.function("kepler_prop")
    d = differentiate_function("kp", kp)
    for k, c in enumerate(("kepler_quarter", "kepler_full", "kepler_back")):
        row, tf = fx[c]["rows"][0], fx[c]["tfs"][0]
        y = np.concatenate([row[:6], [tf - row[6]]])
        assert np.array_equal(y, own["kepler_prop_P"][k])
        J = np.array(evaluate([e for r in d.J for e in r], y)).reshape(6, 7)
        bf, bJ = own["kepler_prop_fB"][k], own["kepler_prop_JB"][k]
        xe, Se, te = fx[c]["x_exact"][0, -1], fx[c]["S_exact"][0][:, :6], fx[c]["dtf_exact"][0]
        cases.close(kp.compute(y), xe.astype(np.longdouble), bf + U * np.abs(xe), c + " value")
        cases.close(J[:, :6], Se.astype(np.longdouble), bJ[:, :6] + U * np.abs(Se), c + " d/d[R, V]")
        cases.close(J[:, 6], te.astype(np.longdouble), bJ[:, 6] + U * np.abs(te), c + " d/d dt")


def test_runtime_modules_with_a_root_compile_without_a_device():
    assert jit.ensure_function(cases.function("kepler_prop"), cases.device_name("kepler_prop"), compile_only=True).startswith("root_kepler_prop_")
    assert jit.ensure_kernel(cases.make_ode(False), "LGL3", False, compile_only=True).startswith("root_newton_")
    assert jit.ensure_event_module(event_cases.make_ode("oscillator"), [cases.event_function()], compile_only=True).startswith("events_oscillator_")
    assert jit.ensure_controller_module(controller_cases.make_ode("pd"), *cases.control_law(), compile_only=True).startswith("ctrl_pd_")


# ---- 7. the twin pair
def test_the_root_ode_and_its_closed_form_twin_agree_through_the_plain_c_builds(tmp_path):
    """The pair of tests/test_gpu_root.py's phase test, on the CPU first: f, J, g, H of the ODE written with the root of s^2 - q and of
    the one written with sqrt(q) sit below a quarter of rel_err < 1e-12."""
    libs = []
    for twin in (False, True):
        d = cases.make_ode(twin).derivatives()
        src = tmp_path / f"ode{int(twin)}.c"
        src.write_text(emit_c(d, "ode"))
        subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", str(src), "-o", str(tmp_path / f"ode{int(twin)}.so"), "-lm"])
        libs.append(C.CDLL(str(tmp_path / f"ode{int(twin)}.so")))
    rng = np.random.default_rng(3)
    worst = 0.0
    fcb, fjcb = cases.ode_callbacks()
    for _ in range(200):
        y = rng.uniform(-2.0, 2.0, 4)
        lam = rng.uniform(-1, 1, 2)
        out = []
        for L in libs:
            f, J, g, H = np.zeros(2), np.zeros((2, 4)), np.zeros(4), np.zeros((4, 4))
            L.ode_fjgh(*[C.c_void_p(a.ctypes.data) for a in (y, lam, f, J, g, H)])
            out.append((f, J, g, H))
        worst = max([worst] + [rel_err(a, b) for a, b in zip(*out)])
        assert np.array_equal(out[0][3], out[0][3].T)
        assert rel_err(out[0][0], fcb(y)) < 1e-13 and rel_err(out[0][1], fjcb(y)[1]) < 1e-13     # (the numpy callbacks of the propagation test)
    print(f"root ODE against its twin: worst rel_err {worst:.3g}")
    assert worst < 0.25 * 1e-12
    g_np, grad_np = cases.event_np()
    K, JK = cases.law_np()
    for _ in range(20):                                                # the event function and the law against their numpy closed forms
        y = rng.uniform(-1.0, 1.0, 3)
        assert abs(cases.event_function().compute(y)[0] - g_np(y)) < 1e-14 and abs(cases.event_function(True).compute(y)[0] - g_np(y)) < 1e-14
        z = rng.uniform(-1.0, 1.0, 2)
        assert abs(cases.control_law()[0].compute(z)[0] - K(z)[0]) < 1e-14
        dl = differentiate_function("law", cases.control_law()[0])
        assert rel_err(np.array(evaluate(list(dl.J[0]), z)), JK(z)[0]) < 1e-13
        de = differentiate_function("ev", cases.event_function())
        assert rel_err(np.array(evaluate(list(de.J[0]), y))[:2], grad_np(y)) < 1e-13
