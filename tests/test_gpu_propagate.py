"""The batched propagation on the device (csrc/propagate_kernels.h through asset_hip_propagate / asset_hip_propagate_stm and
``ode.integrator``) against the 50-digit fixture tests/golden/propagate/propagate.npz and -- where there is no fixture -- against the float64
restatement of tests/propagate_checker.py (each side within its bound of the exact state, so the two are within twice the bound of each
other): every fixture case, the workgroup edges of the batch kernel, the lane-group edges of the STM kernel (a partly filled group,
C = 16 and C = 17, the column-pass path of the 32-state ODE), bitwise equality of the STM call's states with the batch call's and across
the lanes of a group, mixed directions and lengths with a zero-length problem in one wave, a NaN state and the step cap, a run-time
compiled ODE and library ODEs by name."""
import functools

import numpy as np
import pytest

import integ_checker as gck
import propagate_checker as pck
from asset_asrl_amd import synth
from helpers import make_shape, make_vanderpol

pytestmark = pytest.mark.gpu
U = pck.U


@functools.lru_cache(maxsize=None)
def _ode(name):
    from asset_asrl_amd.ode import ODE_LIBRARY
    if name in ODE_LIBRARY:
        return ODE_LIBRARY[name]()
    if name == "vanderpol":
        return make_vanderpol()
    return make_shape(*(int(v) for v in name.split("_")[1:]))


def _integrator(name, opt):
    g = _ode(name).integrator("DOPRI87", opt["def_step"])
    g.setStepSizes(opt["def_step"], opt["min_step"], opt["max_step"])
    g.MaxStepChange, g.Adaptive, g.MaxSteps = opt["max_step_change"], opt["adaptive"], opt["max_steps"]
    g.setAbsTols(np.broadcast_to(opt["abs_tol"], (g.xv,)))
    g.setRelTols(np.broadcast_to(opt["rel_tol"], (g.xv,)))
    return g


def _stm(g, rows, tfs):
    """(xf[m, n], J[m, n, N + 1], steps, status, xf_last) of integrate_stm_parallel(details=True)"""
    res, steps, status, last = g.integrate_stm_parallel(rows, tfs, details=True)
    return np.array([r[0][:g.xv] for r in res]), np.array([r[1] for r in res]), steps, status, last


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


# ---- the fixture
@pytest.mark.parametrize("name", pck.case_names())
def test_device_matches_the_50_digit_fixture(oracle, name):
    c = pck.fixture()[1][name]
    n, uv, pv = c["sizes"]
    N, ns, rows, tfs = n + 1 + uv + pv, c["ns"], c["rows"], c["tfs"]
    opt = pck.case_options(c)
    g = _integrator(c["ode"], opt)
    end, steps, status = g.integrate_parallel(rows, tfs, details=True)
    end = np.array(end)
    assert (status == 0).all(), status
    assert end.shape == (len(tfs), N) and np.array_equal(end[:, n], tfs) and np.array_equal(end[:, n + 1:], rows[:, n + 1:])
    xf, J, steps_s, status_s, last = _stm(g, rows, tfs)
    assert (status_s == 0).all() and np.array_equal(steps_s, steps)
    _same_bits(xf, end[:, :n], "integrate_stm_parallel's end states against integrate_parallel's")
    _same_bits(last, xf, "the last lane of a group against lane 0")
    plain = g.integrate_stm_parallel(rows, tfs)                                       # (asset_hip_propagate_stm itself, without the lanes output)
    _same_bits(np.array([r[0] for r in plain]), end, "integrate_stm_parallel's rows against integrate_parallel's")
    _same_bits(np.array([r[1] for r in plain]), J, "the plain STM entry point against the diagnostic one")
    S = np.concatenate([J[:, :, :n], J[:, :, n + 1:N]], axis=2)
    f = pck.oracle_f(oracle, c["ode"])
    if opt["adaptive"]:
        B = pck.state_bound(c["S_max"], c["steps64_end"][:, 0], opt["abs_tol"])
        pck.compare(end[:, :n], c["x_exact"][:, -1], B, f"{name}: end states")
        gck.compare_step_totals(steps, c["steps64_end"], name)
        pck.compare(S, c["S_exact"], pck.stm_bound(c["S_exact"], c["eS"]), f"{name}: STM")
        b0, bf = pck.time_column_bounds(c["S_exact"], c["eS"], c["f0"], c["Jxf_abs"], B, c["dtf_exact"])
        pck.compare(J[:, :, n], c["dt0_exact"], b0, f"{name}: d xf / d t0")
        pck.compare(J[:, :, N], c["dtf_exact"], bf, f"{name}: d xf / d tf")
    else:
        B = 8.0 * c["d64"] + 16.0 * U * np.abs(c["xld"]).astype(float)
        pck.compare(end[:, :n], c["xld"], B, f"{name}: end states against the longdouble restatement")
        np.testing.assert_array_equal(steps, c["steps64_end"])
        pck.compare(S, c["Sld"], 8.0 * c["dS64"] + 16.0 * U * np.abs(c["Sld"]).astype(float), f"{name}: STM against the longdouble restatement")
        d0, df = pck.time_columns(f, rows, tfs, c["xld"].astype(float), c["Sld"])
        b0, bf = pck.time_column_bounds(c["Sld"].astype(float), 2.0 * c["dS64"].max(axis=(1, 2)), c["f0"], c["Jxf_abs"], B, c["dtf_exact"])
        pck.compare(J[:, :, n], d0, b0, f"{name}: d xf / d t0")
        pck.compare(J[:, :, N], df, bf, f"{name}: d xf / d tf")
    if ns > 1:
        trajs, dsteps, dstatus = g.integrate_dense_parallel(rows, tfs, ns, details=True)
        T = np.array(trajs)
        assert (dstatus == 0).all() and T.shape == (len(tfs), ns, N)
        for i in range(len(tfs)):
            np.testing.assert_array_equal(T[i, :, n], pck.sample_times(rows[i, n], tfs[i], ns))
        assert np.array_equal(T[:, :, n + 1:], np.repeat(rows[:, None, n + 1:], ns, axis=1))
        _same_bits(T[:, 0, :n], rows[:, :n], "sample 0 is x0")
        Bd = pck.state_bound(c["S_max"], c["steps64"][:, 0], opt["abs_tol"])
        pck.compare(T[:, :, :n], c["x_exact"], np.repeat(Bd[:, None, :], ns, axis=1), f"{name}: samples")
        gck.compare_step_totals(dsteps, c["steps64"], name + " dense")
    print(f"{name}: steps {steps.sum(axis=0)} against the restatement's {c['steps64_end'].sum(axis=0)}")


# ---- problems without a fixture: the float64 restatement at twice its bound
class _Problems:
    """m random short arcs of an ODE, the float64 restatement of each computed once on demand"""

    def __init__(self, ode, sizes, m, seed, f, fj, lengths=(0.05, 0.2), mixed=False):
        n = sizes[0]
        named = ode in synth.ODE_SIZES
        self.rows = synth.make_traj(ode, "LGL3", m, seed=seed, T=1.0, sizes=None if named else sizes)[:m].copy()
        rng = np.random.default_rng(seed + 1)
        H = rng.uniform(*lengths, m) * (rng.choice([-1.0, 1.0], m) if mixed else 1.0)
        self.tfs = self.rows[:, n] + H
        self.ode, self.n, self.f, self.fj, self.opt, self._ref = ode, n, f, fj, gck.options(), {}

    def ref(self, i):
        if i not in self._ref:
            r = pck.propagate(self.f, self.fj, self.rows[i], self.tfs[i], 1, self.opt, stm=True)
            assert r["status"] == 0
            self._ref[i] = r
        return self._ref[i]

    def check(self, ids, xf, steps, J=None, what=""):
        n = self.n
        refs = [self.ref(i) for i in ids]
        x64 = np.array([r["xs"][0] for r in refs])
        S64 = np.array([r["S"] for r in refs])
        st64 = np.array([r["steps"] for r in refs])
        S_max = np.maximum(np.abs(S64[:, :, :n]), np.eye(n)[None])
        B = 2.0 * pck.state_bound(S_max, st64[:, 0], self.opt["abs_tol"])
        pck.compare(xf, x64, B, what + ": end states against the restatement")
        gck.compare_step_totals(steps, st64, what)
        if J is not None:
            # Without a 50-digit S the fixture's rule is applied to the restatement: eS, the error of a restated S, is estimated from its
            # own sensitivity to the tolerance -- the local error is proportional to AbsTol, so S(AbsTol) - S(AbsTol / 2) is about half the
            # error of S(AbsTol): eS = 2 max(|S(AbsTol / 2) - S|, |S(2 AbsTol) - S|) -- and each side is within 4 eS + 16 u |S| of the exact
            # one.  Where the step sequence does not depend on the tolerance (a short arc: every step is clamped by MaxStepChange) that
            # estimate is zero and the two differ by rounding alone: the fixed-step rule, 8 dS64 from the longdouble restatement, is added.
            N = J.shape[2] - 1
            S = np.concatenate([J[:, :, :n], J[:, :, n + 1:N]], axis=2)
            eS, dS = np.zeros(len(ids)), np.zeros_like(S64)
            for k, i in enumerate(ids):
                for fac in (0.5, 2.0):
                    o = dict(self.opt, abs_tol=fac * np.asarray(self.opt["abs_tol"]))
                    eS[k] = max(eS[k], 2.0 * np.abs(pck.propagate(self.f, self.fj, self.rows[i], self.tfs[i], 1, o, stm=True)["S"] - S64[k]).max())
                ld = pck.propagate(self.f, self.fj, self.rows[i], self.tfs[i], 1, self.opt, dtype=pck.LD, stm=True)["S"]
                dS[k] = np.abs(S64[k].astype(pck.LD) - ld).astype(float)
            pck.compare(S, S64, 2.0 * pck.stm_bound(S64, eS) + 8.0 * dS, what + ": STM against the restatement")


@functools.lru_cache(maxsize=None)
def _reentry(oracle):
    return _Problems("reentry", (5, 2, 0), 200, 71, pck.oracle_f(oracle, "reentry"), pck.oracle_fj(oracle, "reentry"))


@pytest.mark.parametrize("m", [1, 63, 64, 65, 200])
def test_batch_kernel_workgroup_edges(oracle, m):
    P = _reentry(oracle)
    g = _integrator("reentry", P.opt)
    rows, steps, status = g.integrate_parallel(P.rows[:m], P.tfs[:m], details=True)
    assert (status == 0).all() and len(rows) == m
    ids = np.arange(m) if m < 200 else np.arange(3, 200, 13)
    P.check(ids, np.array(rows)[ids, :5], steps[ids], what=f"reentry x {m}")
    if m == 200:                                                                       # the first 65 are the m = 65 problems: the same lanes' work
        r65 = np.array(g.integrate_parallel(P.rows[:65], P.tfs[:65]))
        _same_bits(np.array(rows)[:65], r65, "a problem's result does not depend on the batch around it")


class _Dual:
    """value and gradient in float64: the Jacobian of the shape ODEs the oracle does not hold"""

    def __init__(self, v, g):
        self.v, self.g = v, g

    def _l(self, o):
        return o if isinstance(o, _Dual) else _Dual(float(o), np.zeros_like(self.g))

    def __add__(self, o):
        o = self._l(o)
        return _Dual(self.v + o.v, self.g + o.g)
    __radd__ = __add__

    def __sub__(self, o):
        o = self._l(o)
        return _Dual(self.v - o.v, self.g - o.g)

    def __rsub__(self, o):
        return self._l(o) - self

    def __mul__(self, o):
        o = self._l(o)
        return _Dual(self.v * o.v, self.g * o.v + o.g * self.v)
    __rmul__ = __mul__


class _DualMath:
    sin = staticmethod(lambda a: _Dual(np.sin(a.v), np.cos(a.v) * a.g))
    cos = staticmethod(lambda a: _Dual(np.cos(a.v), -np.sin(a.v) * a.g))


def _shape_callbacks(n, m, p):
    from golden.make_golden_mesh import ode_shape
    rhs, N = ode_shape(n, m, p), n + 1 + m + p

    def fj(y):
        out = rhs([_Dual(float(y[i]), np.eye(N)[i]) for i in range(N)], _DualMath)
        return np.array([o.v for o in out]), np.array([o.g for o in out])
    return (lambda y: fj(y)[0]), fj


def _stm_problems(oracle, name, m, seed):
    if name.startswith("shape_"):
        sizes = tuple(int(v) for v in name.split("_")[1:])
        f, fj = _shape_callbacks(*sizes)
    else:
        sizes = synth.ODE_SIZES[name]
        f, fj = pck.oracle_f(oracle, name), pck.oracle_fj(oracle, name)
    return _Problems(name, sizes, m, seed, f, fj, lengths=(0.05, 0.12))


STM_EDGES = [("reentry", 1), ("reentry", 7), ("reentry", 8), ("reentry", 9), ("twobody_lt", 3), ("twobody_lt", 4), ("twobody_lt", 5),
             ("shape_10_4_2", 3), ("shape_11_4_2", 3), ("synthetic32", 2)]


@pytest.mark.parametrize("name,m", STM_EDGES, ids=[f"{a}-{b}" for a, b in STM_EDGES])
def test_stm_kernel_lane_group_edges(oracle, name, m):
    """reentry: C = 7 in groups of 8 (one lane idle), 8 problems fill a wave; twobody_lt: C = 9 in groups of 16, 4 problems fill a wave;
    C = 16 fills its group exactly and C = 17 takes a group of 32; synthetic32: groups of 8 lanes walk 32 columns in 4 passes."""
    P = _stm_problems(oracle, name, m, 80 + m)
    g = _integrator(name, P.opt)
    xf, J, steps, status, last = _stm(g, P.rows, P.tfs)
    assert (status == 0).all()
    rows, bsteps, bstatus = g.integrate_parallel(P.rows, P.tfs, details=True)
    _same_bits(xf, np.array(rows)[:, :P.n], "integrate_stm_parallel's end states against integrate_parallel's")
    _same_bits(last, xf, "the last lane of a group against lane 0")
    assert np.array_equal(steps, bsteps)
    P.check(np.arange(m), xf, steps, J, what=f"{name} x {m}")
    N = J.shape[2] - 1
    d0, df = pck.time_columns(P.f, P.rows, P.tfs, xf, np.concatenate([J[:, :, :P.n], J[:, :, P.n + 1:N]], axis=2), dtype=float)
    # the closed forms on the device's own S and xf, so rounding alone: 16 u per term of the sum, and 8 eps_f |f| for the generated
    # right-hand side against the oracle's (eps_f <= 8 u |f|_inf: the margin of tests/mesh_checker.py)
    f0 = np.array([P.f(r) for r in P.rows])
    fscale = 64.0 * U * np.maximum(np.abs(f0).max(axis=1), np.abs(df).max(axis=1))
    b0 = (np.abs(J[:, :, :P.n]) * (16.0 * U * np.abs(f0) + fscale[:, None])[:, None, :]).sum(axis=2)
    pck.compare(J[:, :, P.n], d0, b0, f"{name}: d xf / d t0 is -S_x f(x0) of the device's own S")
    pck.compare(J[:, :, N], df, np.repeat(fscale[:, None], P.n, axis=1), f"{name}: d xf / d tf is f(xf) of the device's own xf")


def test_mixed_directions_and_lengths_with_a_zero_length_problem_in_one_wave(oracle):
    P = _Problems("reentry", (5, 2, 0), 64, 91, pck.oracle_f(oracle, "reentry"), pck.oracle_fj(oracle, "reentry"), lengths=(0.01, 0.4), mixed=True)
    z = 17
    P.tfs[z] = P.rows[z, 5]
    assert (P.tfs > P.rows[:, 5]).any() and (P.tfs < P.rows[:, 5]).any()
    g = _integrator("reentry", P.opt)
    rows, steps, status = g.integrate_parallel(P.rows, P.tfs, details=True)
    rows = np.array(rows)
    assert (status == 0).all() and tuple(steps[z]) == (0, 0)
    _same_bits(rows[z], P.rows[z], "tf == t0 returns the row")
    ids = np.array([i for i in range(64) if i != z])
    P.check(ids[::3], rows[ids[::3], :5], steps[ids[::3]], what="mixed wave")
    dense, dsteps, dstatus = g.integrate_dense_parallel(P.rows[z - 1:z + 2], P.tfs[z - 1:z + 2], 4, details=True)
    assert (dstatus == 0).all() and tuple(dsteps[1]) == (0, 0)
    _same_bits(np.array(dense[1]), np.repeat(P.rows[z][None], 4, axis=0), "tf == t0, dense: every sample is the row")
    xf, J, ssteps, sstatus, _ = _stm(g, P.rows[z - 1:z + 2], P.tfs[z - 1:z + 2])
    assert (sstatus == 0).all() and tuple(ssteps[1]) == (0, 0)
    _same_bits(xf, rows[z - 1:z + 2, :5], "STM call's states")
    assert np.array_equal(J[1, :, :5], np.eye(5)) and np.all(J[1, :, 6:8] == 0.0)
    f0 = P.f(P.rows[z])
    tol = np.full(5, 64.0 * U * np.abs(f0).max())                                      # generated right-hand side against the oracle's
    pck.compare(J[1, :, 8], f0, tol, "tf == t0: d xf / d tf is f(x0)")
    pck.compare(J[1, :, 5], -f0, tol, "tf == t0: d xf / d t0 is -f(x0)")


def test_a_nan_state_and_the_step_cap_do_not_disturb_their_neighbours(oracle):
    P = _Problems("reentry", (5, 2, 0), 10, 95, pck.oracle_f(oracle, "reentry"), pck.oracle_fj(oracle, "reentry"), lengths=(0.03, 0.05))
    opt = gck.options(max_steps=12)
    rows, tfs = P.rows.copy(), P.tfs.copy()
    rows[3, 2] = np.nan
    tfs[5] = rows[5, 5] + 2.0
    ref = [pck.propagate(P.f, P.fj, rows[i], tfs[i], 1, opt) for i in range(10)]
    assert [r["status"] for r in ref] == [0, 0, 0, 2, 0, 1, 0, 0, 0, 0]                 # (the test's own premise)
    good = np.array([0, 1, 2, 4, 6, 7, 8, 9])
    g = _integrator("reentry", opt)
    clean = np.array(g.integrate_parallel(rows[good], tfs[good]))
    out, steps, status = g.integrate_parallel(rows, tfs, details=True)
    out = np.array(out)
    assert status.tolist() == [0, 0, 0, 2, 0, 1, 0, 0, 0, 0]
    assert np.isnan(out[[3, 5], :5]).all() and steps[5].sum() == 12 and steps[3].sum() == 0
    _same_bits(out[good], clean, "the other problems of the batch")
    dense, dsteps, dstatus = g.integrate_dense_parallel(rows, tfs, 5, details=True)
    dense = np.array(dense)
    assert dstatus.tolist() == status.tolist() and np.isnan(dense[5, -1, :5]).all() and np.isnan(dense[3, 1:, :5]).all()
    _same_bits(dense[5, 0, :5], rows[5, :5], "sample 0 of a problem that fails later is x0")
    assert np.isfinite(dense[good]).all()
    xf, J, ssteps, sstatus, _ = _stm(g, rows, tfs)
    assert sstatus.tolist() == status.tolist() and np.isnan(xf[[3, 5]]).all() and np.isnan(J[[3, 5]]).all()
    _same_bits(xf[good], clean[:, :5], "STM call: the other problems of the batch")
    assert np.isfinite(J[good]).all()
    from asset_asrl_amd.integrator import IntegrationError
    with pytest.raises(IntegrationError, match="2 of 10 propagations failed; first: problem 3, status 2"):
        g.integrate_parallel(rows, tfs)


def test_output_times_that_round_to_the_same_double(oracle):
    """|H| / (ns - 1) below the spacing of doubles at t0: a sample whose time is the time already reached is the state as it is."""
    f, fj = pck.oracle_f(oracle, "shape_1_0_0"), pck.oracle_fj(oracle, "shape_1_0_0")
    rows = np.array([[0.7, 1.0], [-0.3, 1.0]])
    tfs = np.array([1.0 + 4 * np.spacing(1.0), 1.0 - 4 * np.spacing(0.5)])
    g = _integrator("shape_1_0_0", gck.options())
    trajs, steps, status = g.integrate_dense_parallel(rows, tfs, 9, details=True)
    T = np.array(trajs)
    assert status.tolist() == [0, 0] and np.isfinite(T).all()
    for i in range(2):
        r = pck.propagate(f, fj, rows[i], tfs[i], 9, gck.options())
        assert r["status"] == 0 and tuple(steps[i]) == r["steps"]
        pck.compare(T[i, :, :1], r["xs"], np.full((9, 1), 64 * U), f"problem {i}: samples against the restatement (steps of a few ulp of t)")
