"""The de Boor mesh-error estimate against 50-digit arithmetic, on the CPU: the fixture tests/golden/mesh_error.npz (written by
tests/golden/make_golden_mesh.py from the formulas and tests/golden/lgl_tables.json) against a known answer, the float64 oracle
(oracle/mesh.cpp) against the fixture under the conditioning-aware bounds of tests/mesh_checker.py, and the device code's scheme
literals (csrc/mesh_kernels.h: mesh_scheme, through the host-side table accessor) against the reference header's, bit for bit."""
import math
import os
import sys

import numpy as np
import pytest

import mesh_checker as mck
from asset_asrl_amd import _lib, synth

MODES = ["Trapezoidal", "LGL3", "LGL5", "LGL7"]
# relative misfit of the 50-digit estimate to the known answer on the committed meshes, the worse of forward and time-reversed (measured
# when the fixture was generated; the test prints it).  The samples are rounded to float64, then divided by h^Order (smallest h 0.07) and
# differenced; LGL7 is limited by the 13- to 15-digit literals of the reference header (their x-weights sum to -2.1e-12, not to zero) and by
# the float64 placement of the interior nodes.
KNOWN_ANSWER_MISFIT = {"Trapezoidal": 1.6e-15, "LGL3": 8.8e-13, "LGL5": 1.1e-9, "LGL7": 3.9e-4}


@pytest.mark.parametrize("mode", MODES)
def test_restatement_reproduces_the_leading_derivative_of_a_polynomial(mode):
    """Known answer for the 50-digit restatement.  For x = P(t) of degree Order + 1 (x' = u = P') the block's Hermite interpolant has
    the leading coefficient y_i = P^(Order) at the block's midpoint on any mesh, so every neighbour difference over (h_i + h_nb) / 2
    is P^(Order+1) and  e_i = |P^(Order+1)|  in every block,  mesh_errors_i = |P^(Order+1)| |h_i|^(Order+1) ErrorWeight.  This pins the
    factorial, the leading weights and both end branches without any transcription.  Asserted at 10 x the misfit measured on the
    committed 7-segment ragged meshes: 1.6e-15 (Trapezoidal), 8.8e-13 (LGL3), 1.1e-9 (LGL5), 3.9e-4 (LGL7)."""
    _, order, ew, _, _, _ = mck.scheme(mode)
    for rev in ("", "-reversed"):
        c = mck.fixture()[1][f"integrator_{mode}_7_poly{rev}"]
        want = math.factorial(order + 1) * abs(c["poly"][-1])
        assert len(c["poly"]) == order + 2 and c["zero_e"] == 0
        h = np.abs(mck.block_widths(c["traj"], mode, 1))
        assert h.max() / h.min() > 3.0                                         # a ragged mesh: h_i + h_nb is not 2 h
        misfit = np.abs(c["e"] / want - 1.0).max()
        want_err = want * np.append(h, h[-1]) ** (order + 1) * ew
        misfit_err = np.abs(c["mesh_errors"][0] / want_err - 1.0).max()
        misfit_dist = np.abs(c["mesh_dist"] / want ** (1.0 / (order + 1)) - 1.0).max()
        print(f"{mode}{rev}: e misfit {misfit:.2e}, mesh_errors {misfit_err:.2e}, mesh_dist {misfit_dist:.2e}")
        assert max(misfit, misfit_err, misfit_dist) <= 10.0 * KNOWN_ANSWER_MISFIT[mode]


def _integrator_traj(mode, coeffs, nb=7, seed=12):
    """x = P(t), u = P'(t) on a ragged mesh over [0, 2], each sample rounded once (summed in longdouble)."""
    import interp_checker as ick
    traj = ick.ragged_traj("integrator", mode, nb, seed=seed, T=2.0, sizes=(1, 1, 0))
    t = traj[:, 1].astype(np.longdouble)
    c = np.asarray(coeffs, dtype=np.longdouble)
    k = np.arange(c.size)
    traj[:, 0] = sum(c[i] * t ** int(i) for i in k).astype(float)
    traj[:, 2] = sum(c[i] * int(i) * t ** int(i - 1) for i in k[1:]).astype(float) if c.size > 1 else 0.0
    return traj


@pytest.mark.parametrize("degree_below", [0, 1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_oracle_estimate_of_a_low_degree_polynomial_is_zero_to_the_bound(oracle, mode, degree_below):
    """For P of degree <= Order the exact y_i is the same constant (or zero) in every block: e = 0.  What the float64 oracle returns is
    rounding alone, and must lie inside the bound tau of the data (eps_f = 0: the integrator's right-hand side is a copy).
    LGL7 is the exception, and not through rounding: the header's decimal weights are not the exact ones (by symmetry of the nodes
    xw_0 = -xw_3 and xw_1 = -xw_2, but the literals miss that by 2.8e-11 and 1.1e-11, more than their last printed digit), so the estimate
    WITH them is not zero -- the 50-digit restatement itself gives 2.8 to 7.8 tau here.  For LGL7 the oracle is therefore held, to the
    same tau, to the 50-digit restatement of this trajectory (which needs mpmath), and the restatement's |e| / tau is printed."""
    _, order, _, _, _, _ = mck.scheme(mode)
    deg = order - degree_below
    coeffs = np.random.default_rng(30 + deg).uniform(-1.0, 1.0, deg + 1)
    for traj in (_integrator_traj(mode, coeffs), _integrator_traj(mode, coeffs)[::-1].copy()):
        rhs = lambda rows: rows[:, 2:3]
        got = oracle.mesh_error_deboor(oracle.get_ode("integrator", 0), oracle.MODES[mode], traj)
        h = mck.block_widths(traj, mode, 1)
        tau = mck.tau_of(*mck.tolerance_data(traj, mode, False, 1, 1, rhs), 0.0)
        zero = np.zeros((1, h.size + 1))
        ref = (mck.estimate(traj, mode, False, 1, 1, rhs)[0], zero, zero, zero)
        if mode == "LGL7":
            pytest.importorskip("mpmath")
            sys.path.insert(0, os.path.dirname(mck.FIXTURE))
            import make_golden_mesh as gen
            ref = gen.estimate_mp("integrator", mode, False, traj)[0]
            print(f"LGL7 degree {deg}: 50-digit |e| / tau <= {(ref[1][:, :-1] / tau).max():.2f} (the header's literals)")
        worst = mck.compare(got, ref, tau, h, mode, what=f"{mode} degree {deg}")
        print(f"{mode} degree {deg}: |e - ref| / tau <= {worst[1]:.3f}")


@pytest.mark.parametrize("name", mck.case_names())
def test_oracle_matches_the_50_digit_fixture(oracle, name):
    c = mck.fixture()[1][name]
    got = oracle.mesh_error_deboor(oracle.get_ode(c["ode"], 0), oracle.MODES[c["mode"]], c["traj"], c["blocked"])
    wt, we, wd = mck.compare_with_fixture(c, got, what=name)
    print(f"{name} [{c['family']}]: worst |got - ref| / bound: tsnd {wt:.3f}, mesh_errors {we:.3f}, mesh_dist {wd:.3f}")


def test_fixture_holds_what_the_issue_lists():
    meta, cases = mck.fixture()
    assert len(cases) == 2 * len(meta["cases"]) and os.path.getsize(mck.FIXTURE) < 1 << 20
    fam = [c["family"] for c in meta["cases"]]
    assert 4 * fam.count("smooth-fine") <= len(fam) and fam.count("random") >= 20 and fam.count("smooth-coarse") >= 6
    assert meta["eps_f_measured"]["integrator"] == 0.0 and meta["eps_f_factor"] == 8.0 and meta["dps"] == 50
    for c in cases.values():
        xv = c["sizes"][0]
        assert c["e"].shape == c["mesh_errors"].shape == c["mesh_dist"].shape == (xv, c["nb"] + 1) and c["tsnd"].shape == (c["nb"] + 1,)
        assert c["tau_s"].shape == (xv, c["nb"]) and c["tau_phi"].shape == (c["nb"],)
        assert np.array_equal(c["e"][:, -1], c["e"][:, -2]) and np.array_equal(c["mesh_errors"][:, -1], c["mesh_errors"][:, -2])
        t = c["traj"][:, xv]
        assert np.all(np.diff(t) < 0) if c["reversed"] else np.all(np.diff(t) > 0)
        tau = mck.tau_of(c["tau_s"], c["tau_phi"], mck.eps_f(c["ode"]))
        e = c["e"][:, :-1]
        assert int((e == 0.0).sum()) == c["zero_e"]
        limit = {"random": 1e-9, "smooth-coarse": 1e-3}.get(c["family"])
        if limit is not None and (e != 0).any():
            assert (tau[e != 0] / e[e != 0]).max() <= limit


@pytest.mark.parametrize("mode", MODES)
def test_device_scheme_literals_equal_the_reference_header(mode):
    """csrc/mesh_kernels.h: mesh_scheme -- Order, ErrorWeight, Order!, the leading power weights -- bit for bit against
    tests/golden/lgl_tables.json (Trapezoidal: the estimator's own literals {0, 0}, {-1, 1}, 2, 1/12, no factorial)."""
    cs, order, ew, F, xw, dxw = mck.scheme(mode)
    got = _lib.lgl_table(cs, "mesh_trapezoidal" if mode == "Trapezoidal" else "mesh")
    assert got.size == 3 + 2 * cs
    np.testing.assert_array_equal(got[:3], [float(order), ew, F])
    np.testing.assert_array_equal(got[3:3 + cs], xw)
    np.testing.assert_array_equal(got[3 + cs:], dxw)


def test_oracle_error_scaling_known_answer_lgl7(oracle):
    """The LGL7 row of tests/test_mesh_error.py: test_oracle_error_scaling_known_answer -- on (sin t, cos t) over [0, 3] halving the mesh
    divides the largest estimate by 2^8.  On 4 and 8 segments, not 40 and 80: at h = 3/40 the terms of y_i are 5040 x 322 x |x| / h^7 =
    1e14, their rounding 1e-2 per unit of e after the division by 2 h -- the estimate of a smooth trajectory is noise there;
    at h = 3/8 the same figure is 1e-9."""
    ode = oracle.get_ode("vanderpol", 0)

    def errors(nseg):
        tc = synth._TC[4]
        edges = np.linspace(0.0, 3.0, nseg + 1)
        t = np.append((edges[:-1, None] + np.asarray(tc[:3])[None, :] * np.diff(edges)[:, None]).ravel(), 3.0)
        traj = np.column_stack([np.sin(t), np.cos(t), t, np.zeros_like(t), np.zeros_like(t)])
        return np.abs(oracle.mesh_error_deboor(ode, oracle.MODES["LGL7"], traj)[1]).max()

    e1, e2 = errors(4), errors(8)
    rate = np.log2(e1 / e2)
    assert abs(rate - 8.0) < 0.35, (e1, e2, rate)


@pytest.mark.parametrize("name", ["reentry_LGL7_3", "twobody_lt_Trapezoidal_blocked_21", "integrator_LGL5_7_poly"])
def test_generator_reproduces_the_committed_case(name):
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_mesh as gen
    meta, cases = mck.fixture()
    spec = next(s for s in gen.SPECS if s["name"] == name)
    assert spec == {k: v for k, v in next(c for c in meta["cases"] if c["name"] == name).items() if k != "zero_e"}
    traj, arrays, zero, _ = gen.make_case(spec)
    for tag, rev in (("fwd", ""), ("rev", "-reversed")):
        c = cases[name + rev]
        np.testing.assert_array_equal(traj[::-1] if rev else traj, c["traj"])
        for k, v in arrays[tag].items():
            np.testing.assert_array_equal(v, c[k], err_msg=f"{name}{rev}: {k}")
        assert zero[int(bool(rev))] == c["zero_e"]
