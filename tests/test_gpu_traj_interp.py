"""The device trajectory table (asset_asrl_amd/interp.py -> asset_hip_traj_table_* -> csrc/interp_kernels.h) against an independent
checker (tests/interp_checker.py: the reference's power weights from tests/golden/lgl_tables.json, the oracle's ODE right-hand
side through ctypes, every sum in numpy.longdouble), and the phase's re-meshing through it.

Value parity is the project's: 1e-10 relative to max(1, |column|max) -- SURVEY's "1e-10 on residuals"; with the same weights a
float64 and a longdouble sum of the degree-7 basis (weights up to 2e3) differ by less than 2e-12.  BlockConstant: controls and
parameters are the block's first row's, their derivative 0 (the derivative of what the table returns)."""
import ctypes as C
import warnings

import numpy as np
import pytest

import interp_checker as ck
from asset_asrl_amd import _lib, synth
from asset_asrl_amd.evaluator import CON
from asset_asrl_amd.interp import LGLInterpTable
from asset_asrl_amd.ode import ShuttleReentry, TwoBody
from helpers import Workload, make_vanderpol

pytestmark = pytest.mark.gpu

TOL = 1e-10
MODES = ["Trapezoidal", "LGL3", "LGL5", "LGL7"]
# (name of the oracle's right-hand side, the ODE handed to the table, sizes for a user ODE, BlockConstant)
CASES = {"reentry": ("reentry", lambda: "reentry", None, False),
         "twobody_lt": ("twobody_lt", lambda: "twobody_lt", None, False),
         "twobody_lt-BlockConstant": ("twobody_lt", lambda: "twobody_lt", None, True),
         "betts_lowthrust": ("betts_lowthrust", lambda: "betts_lowthrust", None, False),
         "vanderpol-jit": ("vanderpol", make_vanderpol, (2, 1, 1), False)}


def _times(traj, xv, K, n, seed):
    t = traj[:, xv]
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(min(t[0], t[-1]), max(t[0], t[-1]), n), t, t[::K], [t[0], t[-1]]])


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "time-reversed"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_values_and_derivatives_match_the_checker(oracle, case, mode, reverse):
    oname, make, sizes, blocked = CASES[case]
    xv = (sizes or synth.ODE_SIZES[oname])[0]
    traj = ck.ragged_traj(oname, mode, 37, seed=41, sizes=sizes)
    if reverse:
        traj = traj[::-1].copy()
    times = _times(traj, xv, ck.MODE_CS[mode] - 1, 3000, 7)
    ref, dref, outside = ck.interpolate(traj, mode, blocked, xv, ck.oracle_rhs(oracle, oname), times)
    assert outside == 0
    with LGLInterpTable(make(), traj, mode, blocked) as table:
        assert (table.T0, table.TF, table.NumBlocks) == (traj[0, xv], traj[-1, xv], 37)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got, dgot = table.InterpolateDeriv(times)
            only = table.Interpolate(times)
            one = table.InterpolateDeriv(float(times[5]))
        assert table.last_outside == 0
    ev, ed = ck.max_rel(got, ref), ck.max_rel(dgot, dref)
    print(f"{case} {mode} reversed={reverse}: value err {ev:.2e}, derivative err {ed:.2e}")
    assert ev < TOL and ed < TOL
    assert np.array_equal(only, got)                                  # with and without the derivative output: the same values
    assert one.shape == (traj.shape[1], 2) and np.array_equal(one[:, 0], got[5]) and np.array_equal(one[:, 1], dgot[5])


@pytest.mark.parametrize("mode", MODES)
def test_polynomials_of_the_tables_degree_are_reproduced(mode):
    """x' = u with u = P'(t): P of degree 2 CS - 1 is the interpolant itself.  1e-10, not tighter: the reference's LGL7 literals
    reproduce their own nodes only to 3.5e-12, and the implementation keeps those literals.  P' is printed, not asserted: the same
    literals limit it to ~1e-12 / h (the longdouble checker itself reaches 7e-10 on this mesh); derivatives are checked against
    the checker in the test above."""
    cs = ck.MODE_CS[mode]
    rng = np.random.default_rng(3)
    P = np.polynomial.Polynomial(rng.uniform(-1.0, 1.0, 2 * cs), domain=[0.0, 2.0], window=[0.0, 1.0])
    traj = ck.ragged_traj("integrator", mode, 11, seed=9, T=2.0, sizes=(1, 1, 0))
    t = traj[:, 1]
    traj[:, 0], traj[:, 2] = P(t), P.deriv()(t)
    tau = np.concatenate([rng.uniform(0.0, 2.0, 2000), t])
    for tr in (traj, traj[::-1].copy()):
        with LGLInterpTable(ck.make_integrator_ode(), tr, mode) as table:
            got, dgot = table.InterpolateDeriv(tau)
        scale, dscale = max(1.0, np.abs(P(tau)).max()), max(1.0, np.abs(P.deriv()(tau)).max())
        e, de = np.abs(got[:, 0] - P(tau)).max() / scale, np.abs(dgot[:, 0] - P.deriv()(tau)).max() / dscale
        print(f"{mode}: P err {e:.2e}, P' err {de:.2e}")
        assert e < TOL
        assert np.abs(got[:, 1] - tau).max() < 1e-14 * 2.0 and np.all(dgot[:, 1] == 1.0)


def test_block_rule_and_out_of_range_queries(oracle):
    mode, xv, K = "LGL5", 6, 2
    traj = ck.ragged_traj("twobody_lt", mode, 9, seed=17)
    tb = traj[::K, xv]
    rhs = ck.oracle_rhs(oracle, "twobody_lt")
    with LGLInterpTable("twobody_lt", traj, mode, blocked=True) as table:
        # BlockConstant controls at an interior boundary: those of the block that ENDS there
        got = table.Interpolate(tb[1:-1])
        assert np.array_equal(got[:, xv + 1:], traj[0:-1 - K:K, xv + 1:])
        assert np.array_equal(table.Interpolate(tb[0])[xv + 1:], traj[0, xv + 1:])
        # outside the data: extrapolated from the end blocks, counted, warned about -- or refused
        out = np.array([tb[0] - 0.3 * (tb[1] - tb[0]), 0.5 * (tb[3] + tb[4]), tb[-1] + 0.2 * (tb[-1] - tb[-2])])
        ref, dref, outside = ck.interpolate(traj, mode, True, xv, rhs, out)
        assert outside == 2
        with pytest.warns(RuntimeWarning, match="outside"):
            got, dgot = table.InterpolateDeriv(out)
        assert table.last_outside == 2
        assert ck.max_rel(got, ref) < TOL and ck.max_rel(dgot, dref) < TOL
        assert np.array_equal(got[0, xv + 1:], traj[0, xv + 1:]) and np.array_equal(got[2, xv + 1:], traj[-1 - K, xv + 1:])
        table.ThrowOutOfBounds = True
        with pytest.raises(ValueError, match="outside"):
            table.Interpolate(out)
        table.ThrowOutOfBounds, table.WarnOutOfBounds = False, False
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            table.Interpolate(out)
    # the C ABI's own input errors (the reference's two checkInput errors, non-finite input): refused, with a message
    dup = traj.copy()
    dup[4, xv] = dup[3, xv]
    back = traj.copy()
    back[5, xv] = back[3, xv] - 1e-3
    for bad, word in ((dup, "duplicate"), (back, "monotonic")):
        with pytest.raises(_lib.AssetHipError, match=word):
            LGLInterpTable("twobody_lt", bad, mode)
    with pytest.raises(_lib.AssetHipError):
        LGLInterpTable("nonexistent_ode_name", traj, mode)


def test_phase_remeshes_through_the_table(oracle):
    from test_gpu_remesh import _check
    traj = Workload("reentry", "LGL7", 200).traj
    rng = np.random.default_rng(23)
    n = 260
    bins = np.concatenate([[0.0], np.sort(rng.uniform(0.0, 1.0, n - 1)), [1.0]])
    bins = np.concatenate([[0.0], np.cumsum(np.maximum(np.diff(bins), 2e-4))])
    bins /= bins[-1]
    ones = np.ones(n, dtype=int)
    ph = ShuttleReentry().phase("LGL7", traj, 200)
    lin = ShuttleReentry().phase("LGL7", traj, 200)
    assert lin.TrajInterpolation == "linear"
    ph.setTrajInterpolation("transcription")
    ph.transcribe()
    first = ph.evaluator
    before = ph.ActiveTraj.copy()
    ph.refineTrajManual(bins, ones)
    lin.refineTrajManual(bins, ones)
    nodes = ck.mesh_times(4, bins, ones, before[0, 5], before[-1, 5])
    ref, _, outside = ck.interpolate(before, "LGL7", False, 5, ck.oracle_rhs(oracle, "reentry"), nodes)
    err = ck.max_rel(ph.ActiveTraj, ref)
    print(f"phase re-meshing against the checker's NDdistribute: {err:.2e}")
    assert outside == 0 and err < TOL
    assert ph.numDefects == lin.numDefects == n and ph._ev is None
    assert np.array_equal(ph.DefBinSpacing, lin.DefBinSpacing) and np.array_equal(ph.DefsPerBin, lin.DefsPerBin)
    assert np.array_equal(ph._nodal_spacing(), lin._nodal_spacing())
    assert np.array_equal(ph.ActiveTraj[:, 5], lin.ActiveTraj[:, 5])
    # the default is np.interp's result, bit for bit, as before
    want = np.column_stack([np.interp(lin.ActiveTraj[:, 5], before[:, 5], before[:, c]) for c in range(8)])
    want[:, 5] = lin.ActiveTraj[:, 5]
    assert np.array_equal(lin.ActiveTraj, want)
    assert np.abs(ph.ActiveTraj - lin.ActiveTraj).max() > 1e-3          # (the two kinds do differ on this data)
    # asset_hip_defect_rebind + evaluation on the new mesh: the oracle's tolerances of tests/test_gpu_remesh.py
    ph.transcribe()
    assert ph.evaluator is first and first.nseg == n
    _check(ph, oracle, 31)
    # returnTrajRange / returnTrajRangeND / returnTrajTable: the exact table of the active trajectory
    cur = ph.ActiveTraj.copy()
    t0, tf = cur[0, 5], cur[-1, 5]
    tl, th = t0 + 0.21 * (tf - t0), t0 + 0.67 * (tf - t0)
    rng_nodes = ck.mesh_times(4, [0.0, 1.0], [7], tl, th)
    ref, _, _ = ck.interpolate(cur, "LGL7", False, 5, ck.oracle_rhs(oracle, "reentry"), rng_nodes)
    got = np.array(ph.returnTrajRange(7, tl, th))
    got_nd = np.array(ph.returnTrajRangeND(7, 0.21, 0.67))
    assert got.shape == (22, 8) and ck.max_rel(got, ref) < TOL and ck.max_rel(got_nd, ref) < TOL
    with ph.returnTrajTable() as table:
        assert table.NumBlocks == n and ck.max_rel(table.InterpRange(7, tl, th), ref) < TOL


def _kepler(t, e=0.4):
    E = np.array(t, dtype=float)
    for _ in range(60):
        E = E - (E - e * np.sin(E) - t) / (1.0 - e * np.cos(E))
    b = np.sqrt(1.0 - e * e)
    r = np.column_stack([np.cos(E) - e, b * np.sin(E), np.zeros_like(E)])
    v = np.column_stack([-np.sin(E), b * np.cos(E), np.zeros_like(E)]) / (1.0 - e * np.cos(E))[:, None]
    return np.column_stack([r, v, t, np.zeros((E.size, 3))])


@pytest.mark.parametrize("mode", ["LGL3", "LGL5", "LGL7"])
def test_hermite_remeshing_leaves_a_hundredth_of_the_linear_residual(mode):
    """Exact samples of a Kepler orbit (e = 0.4, a = 1, mu = 1, no thrust) on 16 equal segments of t in [0, 2], re-distributed on 23:
    max |defect| from the device evaluator on the new mesh.  The CPU restatement gives ratios of 185 (LGL3), 4.4e4, 1.1e7; the bound
    is 100 for all three."""
    res = {}
    for kind in ("linear", "transcription"):
        ph = TwoBody().phase(mode)
        nodes = ph._mesh_times(np.array([0.0, 1.0]), np.array([16]), 0.0, 2.0)
        samples = _kepler(nodes)
        ph.setTraj(samples, 16)
        assert np.abs(ph.ActiveTraj - samples).max() < 1e-15          # setTraj's own linear resampling returns the samples
        ph.setTrajInterpolation(kind)
        ph.refineTrajManual([0.0, 1.0], [23])
        assert ph.numDefects == 23
        res[kind] = float(np.abs(ph.evaluator.eval(CON, ph.solver_input())[0]).max())
    print(f"{mode}: max |CON| linear {res['linear']:.3e}, transcription {res['transcription']:.3e}, "
          f"ratio {res['linear'] / res['transcription']:.3g}")
    assert res["transcription"] * 100.0 <= res["linear"]


def test_resident_table_serves_repeated_device_queries_bitwise():
    import torch
    traj = ck.ragged_traj("reentry", "LGL7", 500, seed=5)
    rng = np.random.default_rng(1)
    ta, tb = rng.uniform(0.0, 10.0, 40000), rng.uniform(0.0, 10.0, 25001)
    L = _lib.lib()

    def dev_query(table, t):
        d_t = torch.from_numpy(t).cuda()
        d_out, d_dout = torch.empty((t.size, 8), dtype=torch.float64, device="cuda"), torch.empty((t.size, 8), dtype=torch.float64, device="cuda")
        d_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        _lib.check(L.asset_hip_traj_table_interp_device(table.handle, C.c_void_p(d_t.data_ptr()), t.size, 1, C.c_void_p(d_out.data_ptr()),
                                                        C.c_void_p(d_dout.data_ptr()), C.c_void_p(d_cnt.data_ptr()), None),
                   "asset_hip_traj_table_interp_device")
        torch.cuda.synchronize()
        assert int(d_cnt.item()) == 0
        return d_out.cpu().numpy(), d_dout.cpu().numpy()

    with LGLInterpTable("reentry", traj, "LGL7") as one:
        a1, b1 = dev_query(one, ta), dev_query(one, tb)           # two queries, one table
        a1_again = dev_query(one, ta)
        host = one.InterpolateDeriv(ta)
    with LGLInterpTable("reentry", traj, "LGL7") as fresh_a:
        a2 = dev_query(fresh_a, ta)
    with LGLInterpTable("reentry", traj, "LGL7") as fresh_b:
        b2 = dev_query(fresh_b, tb)
    for x, y in ((a1, a2), (b1, b2), (a1, a1_again), (a1, host)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def test_a_hundred_thousand_segments_onto_a_hundred_and_thirty_thousand(oracle):
    """100 000 LGL7 segments of `reentry` re-distributed onto 130 000.  The longdouble checker calls the oracle's right-hand side node
    by node from Python, so it covers every 97th query point (4 021 of 390 001, about 1 %) and ALL points of the first and last
    64 blocks; the other 99 % are covered by the same kernel code path only."""
    nb, nn = 100000, 130000
    traj = ck.ragged_traj("reentry", "LGL7", nb, seed=77)
    # the new mesh's node times, formed by the checker.  (The table's own distribute_times differs from them by one unit in the last
    # place at a third of the nodes; on this trajectory of RANDOM states -- O(1) steps between nodes 1e-5 apart -- that alone moves
    # the exact interpolant by 2e-10 relative, so both sides are evaluated at the same times.)
    nodes = ck.mesh_times(4, [0.0, 1.0], [nn], traj[0, 5], traj[-1, 5])
    with LGLInterpTable("reentry", traj, "LGL7") as table:
        out = table.Interpolate(nodes)
        assert table.last_outside == 0
        own = table.NDdistribute([0.0, 1.0], [nn])
        assert table.last_outside == 0 and own.shape == out.shape and np.all(np.isfinite(own))
        assert np.abs(own[:, 5] - nodes).max() <= 1e-14
    assert out.shape == (3 * nn + 1, 8) and np.all(np.isfinite(out))
    tb = traj[::3, 5]
    pick = np.zeros(nodes.size, dtype=bool)
    pick[::97] = True
    pick |= (nodes <= tb[64]) | (nodes >= tb[nb - 64])
    assert pick[::97].sum() >= 1000
    ref, _, outside = ck.interpolate(traj, "LGL7", False, 5, ck.oracle_rhs(oracle, "reentry"), nodes[pick])
    err = ck.max_rel(out[pick], ref)
    print(f"{int(pick.sum())} of {nodes.size} points checked: {err:.2e}")
    assert outside == 0 and err < TOL
