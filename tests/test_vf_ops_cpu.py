"""Every operation of the ``vf`` DSL against a 50-digit reference, on the host: the symbolic rules of vf/ir.py (``Graph.d``, ``_dunary``,
``grad``) walked by ``ir.evaluate``, and the plain-C printer of vf/codegen.py compiled with gcc -- value, Jacobian, adjoint gradient
and adjoint Hessian of the cases of tests/vf_cases.py at all 193 points of the fixture tests/golden/vf_ops.npz (written by
tests/golden/make_golden_vf.py from a second statement of the functions over sympy / mpmath; metric and tolerance: vf_cases.py).
And csrc/asset_math.h, the hand-written sin / cos / tan of every device functor, compiled for the host against the same fixture.

``guarded`` and ``composed`` hold tests that guard a sqrt, a log and a quotient, with points on the other side of the guard and
exactly on it.  Before the reverse sweep of ``Graph.grad`` differentiated a select branch by branch they gave NaN in g and H there
(a zero adjoint times the Inf / NaN local derivative of the branch not taken), and ``ir.evaluate`` raised a math domain error."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vf_cases
from asset_asrl_amd import vf
from asset_asrl_amd.vf import codegen
from asset_asrl_amd.vf.ir import GRAPH as G
from asset_asrl_amd.vf.ir import evaluate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "vf_ops.npz"))
FORMS = [(name, False) for name in vf_cases.CASES] + [("composed", True)]
IDS = [name + ("-flat" if flat else "") for name, flat in FORMS]


def _derivatives(name, flat):
    if flat:
        return vf_cases.build_flat(name)[1]
    return codegen.differentiate_function(name, vf_cases.build(name))


def _roots(d):
    N = d.nin
    return d.f + [e for r in d.J for e in r] + d.g + [d.H[i][j] for i in range(N) for j in range(i + 1)]


def _split(flat, n, N):
    """[napp, n + nN + N + N(N+1)/2] -> {f, J, g, H (lower triangle by rows)}."""
    f, J, g, H = np.split(flat, np.cumsum([n, n * N, N]), axis=1)
    return {"f": f, "J": J.reshape(-1, n, N), "g": g, "H": H}


def check_against_fixture(name, got, cap, d=None, label=""):
    """Every array of `got` against the fixture of case `name`: finite wherever the reference is, per-entry error below 16 x E_ref.
    The figures are printed before they are asserted."""
    worst = {}
    for k, key in enumerate(vf_cases.ARRAYS):
        ref = GOLD[f"{name}_{key}"]
        assert np.all(np.isfinite(ref))
        assert got[key].shape == ref.shape
        assert np.all(np.isfinite(got[key])), f"{label}{name}.{key}: non-finite at rows {sorted(set(np.argwhere(~np.isfinite(got[key]))[:, 0]))[:8]}"
        err = vf_cases.entry_errors(got[key], ref)
        tol = vf_cases.tolerance(GOLD[f"{name}_E_ref"][k], cap)
        worst[key] = (float(err.max()), tol)
        print(f"{label}{name}.{key}: worst error {err.max():.2e} at row {np.unravel_index(err.argmax(), err.shape)[0]}, "
              f"tolerance {tol:.2e} (E_ref {GOLD[f'{name}_E_ref'][k]:.1e})")
    for key, (e, tol) in worst.items():
        assert e <= tol, f"{label}{name}.{key}: {e:.2e} > {tol:.2e}"
    if d is not None:                                   # structural zeros are exact zeros, in the reference too
        N, n = d.nin, d.xv
        for k in range(n):
            for i in range(N):
                if d.J[k][i] is G.zero:
                    assert np.all(GOLD[f"{name}_J"][:, k, i] == 0.0) and np.all(got["J"][:, k, i] == 0.0)
        e = 0
        for i in range(N):
            for j in range(i + 1):
                if d.H[i][j] is G.zero:
                    assert np.all(GOLD[f"{name}_H"][:, e] == 0.0) and np.all(got["H"][:, e] == 0.0)
                e += 1
        for i in range(N):
            if d.g[i] is G.zero:
                assert np.all(GOLD[f"{name}_g"][:, i] == 0.0) and np.all(got["g"][:, i] == 0.0)


@pytest.mark.parametrize("name,flat", FORMS, ids=IDS)
def test_symbolic_rules_match_50_digit_reference(name, flat):
    """``ir.evaluate`` over ``codegen.differentiate_function``: the rules themselves."""
    d = _derivatives(name, flat)
    N, n = d.nin, d.xv
    Y, LAM = GOLD[f"{name}_Y"], GOLD[f"{name}_LAM"]
    roots = _roots(d)
    got = _split(np.array([evaluate(roots, Y[a], LAM[a]) for a in range(Y.shape[0])]), n, N)
    check_against_fixture(name, got, vf_cases.CAP_HOST, d, "evaluate ")
    if name == "composed":
        assert d.chain_rule["form"] == ("flat" if flat else d.chain_rule["form"])
        if not flat:                                   # the block-wise chain rule across the cuts, with a select inside the inner function
            assert d.chain_rule["form"] in ("block", "block_local") and d.chain_rule["ops_" + d.chain_rule["form"]] < d.chain_rule["ops_flat"]
    if name == "bigbody":
        assert d.stats()["ops_fjgh"] > codegen.SPLIT_OPS    # the device functor is emitted in two out-of-line parts


@pytest.mark.parametrize("builder", ["_differentiate_block", "_differentiate_block_local"])
def test_both_block_builders_stay_finite_across_a_select(builder):
    """``differentiate`` keeps the cheaper of the two block-wise forms; here each one on its own against the fixture of `composed`."""
    func = vf_cases.build("composed")
    N, n = func.IRows(), func.ORows()
    ys, lams = [G.var(i) for i in range(N)], [G.lam(k) for k in range(n)]
    f_cut = list(func.outs)
    J, g, H = getattr(codegen, builder)(f_cut, ys, lams)
    roots = G.strip_cuts(f_cut + [e for r in J for e in r] + list(g) + [H[i][j] for i in range(N) for j in range(i + 1)])
    Y, LAM = GOLD["composed_Y"], GOLD["composed_LAM"]
    got = _split(np.array([evaluate(roots, Y[a], LAM[a]) for a in range(Y.shape[0])]), n, N)
    check_against_fixture("composed", got, vf_cases.CAP_HOST, None, builder + " ")


@pytest.mark.parametrize("name,flat", FORMS, ids=IDS)
def test_emitted_c_matches_50_digit_reference(tmp_path, name, flat):
    """``emit_c`` compiled with gcc -O1: the printer (``_Printer._expr``, ``_powi_expr``, ``lower_reciprocals``)."""
    d = _derivatives(name, flat)
    N, n = d.nin, d.xv
    src, so = tmp_path / "c.c", tmp_path / "c.so"
    text = codegen.emit_c(d, "vfc")
    src.write_text(text)
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", str(src), "-o", str(so), "-lm"])
    L = C.CDLL(str(so))
    Y, LAM = GOLD[f"{name}_Y"], GOLD[f"{name}_LAM"]
    napp = Y.shape[0]
    out = np.zeros((napp, n + n * N + N + N * (N + 1) // 2))
    low = [(i, j) for i in range(N) for j in range(i + 1)]
    for a in range(napp):
        y, lam = np.ascontiguousarray(Y[a]), np.ascontiguousarray(LAM[a])
        f, J, g, H = np.zeros(n), np.zeros((n, N)), np.zeros(N), np.full((N, N), np.nan)
        L.vfc_fjgh(*[C.c_void_p(x.ctypes.data) for x in (y, lam, f, J, g, H)])
        assert np.array_equal(H, H.T, equal_nan=True)                   # exactly symmetric
        f1, J1 = np.zeros(n), np.zeros((n, N))                          # the two lower levels print the same values
        L.vfc_fj(*[C.c_void_p(x.ctypes.data) for x in (y, f1, J1)])
        assert np.array_equal(f1, f, equal_nan=True) and np.array_equal(J1, J, equal_nan=True)
        out[a] = np.concatenate([f, J.ravel(), g, [H[i, j] for i, j in low]])
    check_against_fixture(name, _split(out, n, N), vf_cases.CAP_HOST, d, "emit_c ")
    if name == "recip":
        assert text.count("1.0 / ") >= 1 and text.split("vfc_fjgh")[1].count(" / ") < 8     # the shared denominator divides once
    if name == "powers":
        assert "pow(" in text and ") * (" in text                      # powr through pow(), powi through _powi_expr


def test_fixture_covers_what_it_should():
    """193 points per case (a partial wave), every threshold of `guarded` hit exactly and from both sides, neighbours on different
    branches, arctan2 in all four quadrants, arcsin / arccos arguments inside [-0.9, 0.9]."""
    for name, case in vf_cases.CASES.items():
        assert GOLD[f"{name}_Y"].shape == (vf_cases.NAPP, case.N) and GOLD[f"{name}_LAM"].shape == (vf_cases.NAPP, case.n)
        assert vf_cases.NAPP % 64 != 0
        for key in vf_cases.ARRAYS:
            assert np.all(np.isfinite(GOLD[f"{name}_{key}"]))
        for k in range(4):
            vf_cases.tolerance(GOLD[f"{name}_E_ref"][k], vf_cases.CAP_HOST)
            vf_cases.tolerance(GOLD[f"{name}_E_ref"][k], vf_cases.CAP_DEVICE)
    Y = GOLD["guarded_Y"]
    for col, thr in ((0, 0.0), (1, 0.5), (2, 0.0)):
        assert (Y[:, col] == thr).sum() >= 10 and (Y[:, col] > thr).sum() >= 40 and (Y[:, col] < thr).sum() >= 40
    assert np.all(np.diff(np.sign(Y[1:7, 0])) != 0)
    Y = GOLD["piecewise_Y"]
    assert np.all(Y[0::2, 2] > 0) and np.all(Y[1::2, 2] < 0)
    Y = GOLD["inverse_Y"]
    assert {(a > 0, b > 0) for a, b in Y[:, 2:4]} == {(True, True), (True, False), (False, True), (False, False)}
    assert np.abs(0.9 * Y[:, 0] * Y[:, 1]).max() <= 0.9 and np.abs(0.45 * (Y[:, 0] + Y[:, 1])).max() <= 0.9
    assert (GOLD["composed_Y"][:, 0] == 0.0).sum() >= 10


def test_select_is_lazy_on_the_host_and_outermost_in_reverse_mode():
    """``ifelse(x0 > 0, sqrt(x0) * x1, x1 * x2)``: ``compute`` at x0 = -1 returns the false branch and raises nothing; in the printed
    adjoint gradient and Hessian no value of the sqrt branch reaches an output outside a select."""
    a = vf.Arguments(3)
    x0, x1, x2 = a.tolist()
    f = vf.stack([vf.ifelse(x0 > 0.0, vf.sqrt(x0) * x1, x1 * x2), x0 * x1])
    np.testing.assert_array_equal(f.compute([-1.0, 2.0, 3.0]), [6.0, -2.0])
    np.testing.assert_array_equal(f.compute([0.0, 2.0, 3.0]), [6.0, 0.0])
    np.testing.assert_array_equal(f.compute([4.0, 2.0, 3.0]), [4.0, 8.0])
    d = codegen.differentiate_function("guard1", f)
    for y in ([-1.0, 2.0, 3.0], [0.0, 2.0, 3.0]):
        vals = evaluate(_roots(d), y, [0.5, -2.0])
        assert np.all(np.isfinite(vals))
    g0 = evaluate([d.g[0], d.H[0][0], d.H[1][0]], [-1.0, 2.0, 3.0], [0.5, -2.0])
    assert g0 == [-4.0, 0.0, -2.0]
    g1 = evaluate([d.g[0], d.H[0][0], d.H[1][0]], [4.0, 2.0, 3.0], [0.5, -2.0])
    np.testing.assert_allclose(g1, [0.5 * 2.0 * 0.25 - 4.0, -0.5 * 2.0 * 0.25 / 8.0, 0.5 * 0.25 - 2.0], rtol=1e-15)


def test_condition_has_no_truth_value():
    """``0.0 < x < 1.0`` and ``(a > b) and (c < d)`` go through ``bool()``: Python would keep one test and drop the other silently."""
    a = vf.Arguments(2)
    x, y = a.tolist()
    with pytest.raises(TypeError, match="use & / | to join conditions"):
        0.0 < x < 1.0
    with pytest.raises(TypeError, match="use & / | to join conditions"):
        (x > y) and (y < 1.0)
    with pytest.raises(TypeError):
        bool(x > 0.0)
    both, either = (x > 0.0) & (y < 1.0), (x > 0.0) | (y < 1.0)
    assert both.compute([1.0, 0.0]) and not both.compute([1.0, 2.0])
    assert either.compute([1.0, 2.0]) and not either.compute([-1.0, 2.0])
    np.testing.assert_array_equal(vf.ifelse(both, x, y).compute([1.0, 0.5]), [1.0])


# --------------------------------------------------------------------------- csrc/asset_math.h on the host

_DRIVER = r"""
#include <cstdio>
#include "asset_math.h"
int main() {
  double x;
  while (std::scanf("%la", &x) == 1) {
    double s, c;
    asset_sincos(x, &s, &c);
    std::printf("%a %a %a %a %a\n", asset_sin(x), asset_cos(x), asset_tan(x), s, c);
  }
  return 0;
}
"""


def am_reference(which):
    return GOLD[f"am_{which}_hi"], GOLD[f"am_{which}_lo"].astype(float)


def check_asset_math(x, s, c, t, label=""):
    """The bounds of csrc/asset_math.h: sin and cos within 2e-16 absolute while the products of the reduction are exact
    (|x| < 2^19 pi/2), 2e-16 + |x| 2^-53 beyond -- the header's own claim; tan, one quotient of two results each good to 2 ulp,
    within 4 ulp.  The reference is a double plus a float32 remainder, so the comparison itself loses nothing."""
    x = np.asarray(x)
    inside = np.abs(x) < vf_cases.AM_EXACT_RANGE
    bound = np.where(inside, vf_cases.AM_ABS, vf_cases.AM_ABS + np.abs(x) * 2.0 ** -53)
    ok = True
    for nm, got in (("sin", s), ("cos", c), ("tan", t)):
        hi, lo = am_reference(nm)
        assert np.all(np.isfinite(got)), f"{label}asset_{nm}: non-finite"
        err = np.abs((got - hi) - lo)
        ulps = err / np.spacing(np.abs(hi))
        for k, sname in enumerate(GOLD["am_set_names"]):
            m = GOLD["am_set"] == k
            print(f"{label}asset_{nm} {sname}: worst absolute error {err[m].max():.3e}, {ulps[m].max():.2f} ulp")
        ok = ok and bool(np.all(ulps <= vf_cases.AM_TAN_ULP) if nm == "tan" else np.all(err <= bound))
    assert ok


def test_asset_math_host_build_matches_50_digit_reference(tmp_path):
    src, exe = tmp_path / "am.cpp", tmp_path / "am"
    src.write_text(_DRIVER)
    subprocess.check_call(["g++", "-O2", "-I", os.path.join(ROOT, "asset_asrl_amd", "csrc"), str(src), "-o", str(exe)])

    def run(xs):
        out = subprocess.run([str(exe)], input="\n".join(float(v).hex() for v in xs) + "\n", capture_output=True, text=True, check=True)
        return np.array([[float.fromhex(w) for w in ln.split()] for ln in out.stdout.splitlines()])
    x = GOLD["am_x"]
    r = run(x)
    assert r.shape == (x.size, 5)
    assert np.array_equal(r[:, 0], r[:, 3]) and np.array_equal(r[:, 1], r[:, 4])        # asset_sin / asset_cos are asset_sincos
    check_asset_math(x, r[:, 0], r[:, 1], r[:, 2], "host ")
    z = run([0.0, -0.0, float("nan"), float("inf"), float("-inf")])
    assert z[0, 0] == 0.0 and not np.signbit(z[0, 0]) and z[1, 0] == 0.0 and np.signbit(z[1, 0])     # sin(-0.0) is -0.0
    assert z[0, 1] == 1.0 and z[1, 1] == 1.0 and np.signbit(z[1, 2])
    assert np.all(np.isnan(z[2:, :3]))                                                              # NaN and +-Inf give NaN
