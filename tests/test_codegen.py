"""CPU tests of the ODE front end + symbolic differentiation + code printers against the oracle's independent
AD2 derivatives of independently written right-hand sides."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from asset_asrl_amd import ode as odelib
from asset_asrl_amd import synth, vf
from asset_asrl_amd.vf.codegen import emit_c, emit_hip_functor
from asset_asrl_amd.vf.ir import evaluate
from helpers import Workload, rel_err


def _point(name, seed=3):
    w = Workload(name, "LGL3", 3, seed=seed)
    xv, uv, pv = synth.ODE_SIZES[name]
    return w.traj[1].copy()


@pytest.mark.parametrize("name", list(odelib.ODE_LIBRARY))
def test_symbolic_derivatives_match_oracle_ad2(oracle, name):
    d = odelib.ODE_LIBRARY[name]().derivatives()
    o = oracle.get_ode(name, 0)
    N, n = d.nin, d.xv
    y = _point(name)
    lam = np.random.default_rng(1).uniform(-1, 1, n)
    f = np.zeros(n)
    J = np.zeros((n, N))
    g = np.zeros(N)
    H = np.zeros((N, N))
    fn = C.CFUNCTYPE(None, *([C.c_void_p] * 7))(o.fjgh)
    fn(y.ctypes.data, lam.ctypes.data, f.ctypes.data, J.ctypes.data, g.ctypes.data, H.ctypes.data, o.ctx)
    assert rel_err(evaluate(d.f, y), f) < 1e-13
    assert rel_err(np.array(evaluate([e for r in d.J for e in r], y)).reshape(n, N), J) < 1e-12
    assert rel_err(evaluate(d.g, y, lam), g) < 1e-12
    Hs = np.array(evaluate([d.H[i][j] for i in range(N) for j in range(N)], y, lam)).reshape(N, N)
    Hs = np.tril(Hs) + np.tril(Hs, -1).T
    assert rel_err(Hs, H) < 1e-12


def test_emitted_c_compiles_and_matches_dag(tmp_path):
    o = odelib.ShuttleReentry()
    d = o.derivatives()
    src = tmp_path / "r.c"
    src.write_text(emit_c(d, "ode_r"))
    so = tmp_path / "r.so"
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", str(src), "-o", str(so), "-lm"])
    L = C.CDLL(str(so))
    y = _point("reentry")
    lam = np.arange(1.0, 6.0)
    f, J, g, H = np.zeros(5), np.zeros((5, 8)), np.zeros(8), np.zeros((8, 8))
    L.ode_r_fjgh(*[C.c_void_p(a.ctypes.data) for a in (y, lam, f, J, g, H)])
    assert rel_err(f, evaluate(d.f, y)) < 1e-14
    assert rel_err(g, evaluate(d.g, y, lam)) < 1e-13
    assert np.abs(H - H.T).max() == 0.0
    hip = emit_hip_functor(d, "OdeR")
    assert "struct OdeR" in hip
    # the functor carries the operation count of its second-derivative body: csrc/defect_resident.h decides by it whether the looped
    # kernel of the shape is also built as two-wave workgroups (ResDims::LOOP_PAIR: heavy right-hand sides only)
    assert f"static constexpr int OPS_FJGH = {d.stats()['ops_fjgh']};" in hip and d.stats()["ops_fjgh"] >= 300
    assert odelib.TwoBody().derivatives().stats()["ops_fjgh"] < 300


def test_dsl_surface_and_errors():
    X = vf.Arguments(4)
    a, b = X.head(2), X.tail(2)
    np.testing.assert_allclose((a.dot(b) * 2.0 + 1).compute([1, 2, 3, 4]), [23.0])
    np.testing.assert_allclose(X.head3().cross(X.tail3()).compute([1, 0, 0, 1]), [0, -1, 0])
    np.testing.assert_allclose(vf.stack(a.norm(), b.normalized()).compute([3, 4, 0, 2]), [5, 0, 1])
    F = vf.stack(vf.sin(X[0]), X[1] ** 2)
    G = vf.Arguments(2)
    np.testing.assert_allclose((G[0] + G[1])(F).compute([0.5, 3, 0, 0]), [np.sin(0.5) + 9])
    with pytest.raises(ValueError):
        X.segment(3, 2)
    with pytest.raises(ValueError):
        vf.Arguments(3).eval(vf.Arguments(2))
    with pytest.raises(ValueError):
        odelib.ODEBase(vf.Arguments(5).head(2), 3, 1)      # output rows != Xvars
    args = odelib.ODEArguments(3, 2, 1)
    assert args.IRows() == 7 and args.UVec().ORows() == 2 and args.PVar(0).ORows() == 1
    np.testing.assert_allclose(args.TVar().compute(np.arange(7.0)), [3.0])


def test_block_chain_rule_across_compositions():
    """Expressions that are COMPOSED, ``outer(inner(y))``, keep cuts at the inner function's outputs (vf/ir.py: Graph.cut) and are
    differentiated block-wise across them (vf/codegen.py: _differentiate_block -- the reference's NestedFunction chain rule,
    CommonFunctions/NestedFunction.h:140-270): the same J, g, H as the flattened expression to rounding, in fewer operations; the
    builder keeps the cheaper of the two forms and what it returns holds no cuts."""
    from asset_asrl_amd.vf import codegen
    from asset_asrl_amd.vf.ir import topo_order
    from helpers import make_nested_orbit
    ode = make_nested_orbit()
    assert any(n.op == "cut" for n in topo_order(ode.func.outs))
    d = ode.derivatives()
    assert d.chain_rule["form"] in ("block", "block_local")        # (total Jacobians of the cuts / local elimination: the cheaper)
    assert min(d.chain_rule["ops_block"], d.chain_rule["ops_block_local"]) < 0.92 * d.chain_rule["ops_flat"]
    assert d.stats()["ops_fjgh"] == d.chain_rule["ops_" + d.chain_rule["form"]]
    N, n = d.nin, d.xv
    roots = d.f + [e for r in d.J for e in r] + d.g + [d.H[i][j] for i in range(N) for j in range(i + 1)]
    assert not any(x.op in ("cut", "frozen") for x in topo_order(roots))
    old = codegen.BLOCK_CHAIN_RULE
    codegen.BLOCK_CHAIN_RULE = False
    try:
        d0 = codegen.differentiate("flat", ode.func, 4, 1, 1)
    finally:
        codegen.BLOCK_CHAIN_RULE = old
    assert d0.chain_rule["form"] == "flat" and d0.stats()["ops_fjgh"] == d.chain_rule["ops_flat"]
    roots0 = d0.f + [e for r in d0.J for e in r] + d0.g + [d0.H[i][j] for i in range(N) for j in range(i + 1)]
    rng = np.random.default_rng(7)
    for _ in range(5):
        y = np.concatenate([rng.uniform(0.6, 1.4, 1), rng.uniform(-1, 1, N - 1)])
        y[2] = rng.uniform(0.2, 0.9)
        lam = rng.uniform(-1, 1, n)
        a, b = np.array(evaluate(roots, y, lam)), np.array(evaluate(roots0, y, lam))
        assert np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))) < 1e-13
    # the structure is the same whichever way it was formed
    assert d.stats()["nnz_J"] == d0.stats()["nnz_J"] and d.stats()["nnz_H_lower"] == d0.stats()["nnz_H_lower"]
    # ... and finite differences of the composed function agree with its Jacobian
    y = np.array([1.1, 0.4, 0.5, -0.3, 0.7, 0.2, 1.5])
    J = np.array(evaluate([e for r in d.J for e in r], y)).reshape(n, N)
    for i in range(N):
        e = np.zeros(N); e[i] = 1e-6
        fd = (ode.func.compute(y + e) - ode.func.compute(y - e)) / 2e-6
        assert np.max(np.abs(fd - J[:, i])) < 1e-7


def test_an_explicit_cut_is_the_identity_and_a_barrier():
    """``.cut()``: numerically the identity; for ir.Graph.d / grad a variable of its own (partial derivatives)."""
    from asset_asrl_amd.vf.ir import GRAPH as G
    a = vf.Arguments(3)
    inner = (a[0] * a[1] + vf.sin(a[2])).cut()
    f = inner * inner + a[0]
    y = np.array([0.3, -1.2, 0.8])
    assert abs(f.compute(y)[0] - ((y[0] * y[1] + np.sin(y[2])) ** 2 + y[0])) < 1e-15
    c = inner.outs[0]
    assert c.op == "cut"
    assert G.d(f.outs[0], G.var(1)) is G.zero                       # nothing flows through the cut
    assert abs(evaluate([G.d(f.outs[0], c)], y)[0] - 2 * (y[0] * y[1] + np.sin(y[2]))) < 1e-15
    assert G.d(f.outs[0], G.var(0)) is G.one                        # the direct dependence only
    assert vf.Arguments(2)[0].cut().outs[0].op == "var"             # plain arguments are never cut


def test_conditionals_abs_and_sign_match_oracle_ad2(oracle):
    """``vf.ifelse`` (tests joined by ``&``, a test of the time), ``vf.abs``, ``vf.sign`` -- the reference's IfElseFunction,
    ConditionalStatement and SignFunction (CommonFunctions/Conditional.h:19-260): value, Jacobian, adjoint gradient and adjoint Hessian
    are those of the branch the test picks.  Against the oracle's AD2 derivatives of the same right-hand side written with plain C++
    branches (oracle/odes.h: switched), at points on every side of every test."""
    from helpers import make_switched
    ode = make_switched()
    d = ode.derivatives()
    o = oracle.get_ode("switched", 0)
    N, n = d.nin, d.xv
    rng = np.random.default_rng(0)
    sides = set()
    fn = C.CFUNCTYPE(None, *([C.c_void_p] * 7))(o.fjgh)
    for _ in range(300):
        y = rng.uniform(-1, 1, N)
        y[2] = rng.uniform(0, 10)
        lam = rng.uniform(-1, 1, n)
        sides.add((y[0] > 0.25 and y[1] >= 0.0, y[2] < 5.0, y[1] > 0))
        f, J, g, H = np.zeros(n), np.zeros((n, N)), np.zeros(N), np.zeros((N, N))
        fn(y.ctypes.data, lam.ctypes.data, f.ctypes.data, J.ctypes.data, g.ctypes.data, H.ctypes.data, o.ctx)
        assert rel_err(evaluate(d.f, y), f) < 1e-14
        assert rel_err(np.array(evaluate([e for r in d.J for e in r], y)).reshape(n, N), J) < 1e-13
        assert rel_err(evaluate(d.g, y, lam), g) < 1e-13
        Hs = np.array(evaluate([d.H[max(i, j)][min(i, j)] for i in range(N) for j in range(N)], y, lam)).reshape(N, N)
        assert rel_err(Hs, H) < 1e-13
    assert len(sides) == 6                     # (every reachable combination: the stiff branch needs x1 >= 0)
    # the printers: a condition is printed inside its select, in C and in the device functor
    assert "? " in emit_c(d, "ode_switched") and "&&" in emit_hip_functor(d, "OdeSwitched")
    with pytest.raises(ValueError):
        vf.ifelse(vf.Arguments(2)[0], 1.0, 2.0)                       # the test must be a comparison


def test_guarded_branches_match_oracle_ad2(oracle):
    """Conditionals that GUARD a sqrt, a log and a quotient: on the other side of the test, and exactly on it, the branch that is not
    taken is NaN / -Inf / a division by zero, and nothing of it may reach J, g or H -- the select stays outermost in the reverse sweep
    too (vf/ir.py: Graph.grad), as the reference's IfElseFunction evaluates the taken branch only.  Against the oracle's AD2 derivatives
    of the same right-hand side with plain C++ branches (oracle/odes.h: guarded), through ``ir.evaluate`` and through the compiled C."""
    from helpers import make_guarded
    ode = make_guarded()
    d = ode.derivatives()
    o = oracle.get_ode("guarded", 0)
    N, n = d.nin, d.xv
    with tempfile.TemporaryDirectory() as tmp:
        src, so = os.path.join(tmp, "g.c"), os.path.join(tmp, "g.so")
        with open(src, "w") as fh:
            fh.write(emit_c(d, "ode_guarded"))
        subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", src, "-o", so, "-lm"])
        L = C.CDLL(so)
        rng = np.random.default_rng(5)
        fn = C.CFUNCTYPE(None, *([C.c_void_p] * 7))(o.fjgh)
        sides = set()
        for k in range(300):
            y = rng.uniform(-1, 1, N)
            y[1] = rng.uniform(-0.5, 1.5)
            if k % 5 == 0:
                y[0] = 0.0
            if k % 7 == 0:
                y[1] = 0.5
            if k % 6 == 0:
                y[3] = 0.0
            lam = rng.uniform(-1, 1, n)
            sides.add((float(np.sign(y[0])), float(np.sign(y[1] - 0.5)), float(np.sign(y[3]))))
            f, J, g, H = np.zeros(n), np.zeros((n, N)), np.zeros(N), np.zeros((N, N))
            fn(y.ctypes.data, lam.ctypes.data, f.ctypes.data, J.ctypes.data, g.ctypes.data, H.ctypes.data, o.ctx)
            assert all(np.all(np.isfinite(a)) for a in (f, J, g, H))
            Hs = evaluate([d.H[max(i, j)][min(i, j)] for i in range(N) for j in range(N)], y, lam)
            got = (evaluate(d.f, y), evaluate([e for r in d.J for e in r], y), evaluate(d.g, y, lam), Hs)
            f2, J2, g2, H2 = np.zeros(n), np.zeros((n, N)), np.zeros(N), np.zeros((N, N))
            L.ode_guarded_fjgh(*[C.c_void_p(a.ctypes.data) for a in (y, lam, f2, J2, g2, H2)])
            for a, b, c, tol in zip(got, (f2, J2, g2, H2), (f, J, g, H), (1e-14, 1e-13, 1e-13, 1e-13)):
                assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
                assert rel_err(np.asarray(a).reshape(c.shape), c) < tol and rel_err(b, c) < tol
        assert len(sides) == 27                        # below, on and above every guard, in every combination
