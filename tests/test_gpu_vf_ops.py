"""Every operation of the ``vf`` DSL on the device against a 50-digit reference: the cases of tests/vf_cases.py compiled at run time
into function kernels (csrc/func_kernels.h), one application per stored point of tests/golden/vf_ops.npz, all five evaluation kinds,
per entry in the metric of vf_cases.py; csrc/asset_math.h in its device build; and an ODE whose conditionals guard a sqrt, a log and a
quotient through the defect kernels (the f_save / fjgh_load route the function kernels do not take) against the oracle."""
import contextlib

import numpy as np
import pytest

import vf_cases
from asset_asrl_amd import jit, vf
from asset_asrl_amd.evaluator import (CON, CON_ADJGRAD, JAC, JAC_ADJGRAD, JAC_ADJGRAD_HESS, DefectEvaluator,
                                      unpack_kkt_block)
from asset_asrl_amd.pathfuncs import FunctionEvaluator
from test_gpu_parity import _check_blocks
from test_vf_ops_cpu import GOLD, check_against_fixture, check_asset_math

pytestmark = pytest.mark.gpu
KINDS = (JAC_ADJGRAD_HESS, CON, CON_ADJGRAD, JAC, JAC_ADJGRAD)
WITH_L = (CON_ADJGRAD, JAC_ADJGRAD, JAC_ADJGRAD_HESS)


def _identity_tables(napp, N, n):
    """One application is one stored point: no variable and no row is shared."""
    return (np.arange(napp * N, dtype=np.int32).reshape(napp, N), np.arange(napp * n, dtype=np.int32).reshape(napp, n))


def _unpack(kkt, N, n):
    """KKT blocks -> (J[napp, n, N], H lower triangle by rows [napp, N(N+1)/2]); H is exactly symmetric by construction."""
    low = [(i, j) for i in range(N) for j in range(i + 1)]
    J, H = np.empty((kkt.shape[0], n, N)), np.empty((kkt.shape[0], len(low)))
    for a in range(kkt.shape[0]):
        Ha, Ja = unpack_kkt_block(kkt[a], N, n)
        J[a], H[a] = Ja, [Ha[i, j] for i, j in low]
    return J, H


@pytest.mark.parametrize("name,flat", vf_cases.DEVICE_FORMS, ids=[n + ("-flat" if f else "") for n, f in vf_cases.DEVICE_FORMS])
def test_dsl_operations_on_the_device_match_50_digit_reference(name, flat):
    case = vf_cases.CASES[name]
    N, n = case.N, case.n
    Y, LAM = GOLD[f"{name}_Y"], GOLD[f"{name}_LAM"]
    napp = Y.shape[0]
    vindex, cindex = _identity_tables(napp, N, n)
    with (vf_cases.flat_chain_rule() if flat else contextlib.nullcontext()):
        ev = FunctionEvaluator(vf_cases.build(name), vf_cases.device_name(name, flat), vindex, cindex, napp * N, napp * n)
    assert (ev.IR, ev.OR) == (N, n)
    X, L = Y.ravel().copy(), LAM.ravel().copy()
    for what in KINDS:
        fx, agx, kkt = ev.eval(what, X, L if what in WITH_L else None)
        got = {"f": np.asarray(fx).reshape(napp, n)}
        if what in WITH_L:
            got["g"] = np.asarray(agx).reshape(napp, N)
        if what >= JAC:
            got["J"], H = _unpack(np.asarray(kkt).reshape(napp, -1), N, n)
            if what == JAC_ADJGRAD_HESS:
                got["H"] = H
        for key in vf_cases.ARRAYS:                   # what a kind does not compute is not compared
            got.setdefault(key, GOLD[f"{name}_{key}"])
        check_against_fixture(name, got, vf_cases.CAP_DEVICE, None, f"device kind {what} ")
    ev.close()


def test_asset_math_device_build_matches_50_digit_reference():
    """``stack(sin x0, cos x1, tan x2)`` with x0 = x1 = x2 over the argument sets of the fixture: the value body calls asset_sin,
    asset_cos and asset_tan; the diagonal of the Jacobian gives cos, -sin (through asset_sincos: the derivative pairs with the value)
    and 1 + tan^2.  The bounds of the host test; 1 + tan^2 squares a result good to 4 ulp -- 8 ulp -- and rounds twice more and the
    stored reference once: 10.5 ulp."""
    x = GOLD["am_x"]
    napp = x.size
    vindex, cindex = _identity_tables(napp, 3, 3)
    ev = FunctionEvaluator(vf_cases.trig3(vf.Arguments(3)), "vfops_trig3", vindex, cindex, napp * 3, napp * 3)
    X = np.repeat(x, 3)
    fx, _, _ = ev.eval(CON, X, None)
    fx = np.asarray(fx).reshape(napp, 3)
    check_asset_math(x, fx[:, 0], fx[:, 1], fx[:, 2], "device value body ")
    assert np.signbit(fx[[k for k, v in enumerate(x) if v == 0.0 and np.signbit(v)], 0]).all()      # sin(-0.0) is -0.0
    fx2, _, kkt = ev.eval(JAC, X, None)
    fx2 = np.asarray(fx2).reshape(napp, 3)
    J, _ = _unpack(np.asarray(kkt).reshape(napp, -1), 3, 3)
    assert np.all(np.isfinite(J))
    check_asset_math(x, fx2[:, 0], fx2[:, 1], fx2[:, 2], "device Jacobian body ")
    check_asset_math(x, -J[:, 1, 1], J[:, 0, 0], fx2[:, 2], "device Jacobian diagonal ")
    sec2 = GOLD["am_sec2"]
    ulps = np.abs(J[:, 2, 2] - sec2) / np.spacing(sec2)
    print(f"device 1 + tan^2: worst error {ulps.max():.2f} ulp")
    assert ulps.max() <= 2.0 * vf_cases.AM_TAN_ULP + 2.5
    for i, j in ((0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)):
        assert np.all(J[:, i, j] == 0.0)
    Xn = np.repeat(np.array([np.nan, np.inf, -np.inf]), 3)                                       # NaN and +-Inf give NaN
    v3, c3 = _identity_tables(3, 3, 3)
    ev.close()
    ev = FunctionEvaluator(vf_cases.trig3(vf.Arguments(3)), "vfops_trig3", v3, c3, 9, 9)
    fn, _, _ = ev.eval(CON, Xn, None)
    assert np.all(np.isnan(np.asarray(fn)))
    ev.close()


@pytest.mark.parametrize("mode,blocked", [("LGL5", False), ("LGL7", True), ("Trapezoidal", False)])
def test_user_ode_with_guarded_branches_matches_oracle(oracle, mode, blocked):
    """Conditionals that guard a sqrt, a log and a quotient in an ODE, through the defect kernels (value pass saving its transcendental
    values, second-derivative pass loading them: f_save / fjgh_load), with states on both sides of every guard and exactly on it:
    every output finite, and equal to the oracle's AD2 derivatives of the same right-hand side with plain C++ branches."""
    from helpers import guarded_workload, make_guarded
    name = jit.ensure_kernel(make_guarded(), mode, blocked)
    w = guarded_workload(mode, blocked)
    nlp = oracle.Nlp(oracle.get_ode("guarded", 0), oracle.MODES[mode], w.blocked, w.vindex, w.cindex, w.n_primal, w.n_equal, 2)
    ev = DefectEvaluator(name, mode, w.blocked, w.vindex, w.cindex, w.n_primal, w.n_equal)
    for what in KINDS:
        ref = nlp.eval_blocks(what, w.X, w.L)
        got = ev.eval(what, w.X, w.L if what in WITH_L else None)
        for a, b in zip(got, ref):
            if b is not None and a is not None:
                assert np.all(np.isfinite(b)), "the oracle itself is not finite: the workload is wrong"
                assert np.all(np.isfinite(a))
        _check_blocks(got, ref, w, what)
    ev.close()
