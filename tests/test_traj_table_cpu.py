"""CPU tests of the per-entry trajectory-table fixtures (tests/golden/traj_table/, tests/traj_table_checker.py): the float64 model of
the documented algorithm stays inside an eighth of the bound on every entry (that is where the two kappa come from) and reproduces
every E = 0 entry exactly; blocks and outside counts agree with tests/interp_checker.py; every case holds its query kinds; the
generator reproduces a stored file bit for bit; and the fixture has teeth -- five mutations of the model each put an entry of a named
case over its bound."""
import io
import os
import sys

import numpy as np
import pytest

import interp_checker as ick
import traj_table_checker as tc

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = tc.all_cases()


@pytest.fixture(scope="module")
def gen():
    sys.path.insert(0, GOLDEN)
    import make_golden_traj_table as g
    return g


def test_fixture_holds_the_cases_of_the_generator_under_the_size_cap(gen):
    assert CASES == sorted(c["name"] for c in gen.cases())
    cap = os.path.getsize(gen.SIZE_CAP_FILE)
    for name in CASES:
        f = tc.load(name)
        assert os.path.getsize(os.path.join(tc.DIR, name + ".npz")) < cap
        nq, N = f["times"].size, f["N"]
        assert f["traj"].dtype == f["times"].dtype == np.float64 and f["traj"].shape == (f["nb"] * f["K"] + 1, N)
        assert sum(f["meta"]["sizes"]) + 1 == N and f["meta"]["nb"] == f["nb"]
        for k in tc.KINDS:
            assert f[k].dtype == np.float64 and f[k + "E"].dtype == np.float32 and f[k].shape == f[k + "E"].shape == (nq, N)
            assert np.all(np.isfinite(f[k])) and np.all(np.isfinite(f[k + "E"])) and np.all(f[k + "E"] >= 0)
    # the edges the cases are there for
    shape = lambda n: (tc.load(n)["traj"].shape[0], tc.load(n)["nb"])
    assert shape("brachistochrone_Trapezoidal_nodes64") == (64, 63) and shape("brachistochrone_Trapezoidal_nodes65") == (65, 64)
    assert shape("brachistochrone_LGL5_nodes65") == (65, 32)
    assert shape("brachistochrone_LGL7_nodes64") == (64, 21) and shape("brachistochrone_LGL7_nodes67") == (67, 22)
    assert [shape(f"reentry_{m}_nb{n}")[1] for m in ("LGL3", "LGL7") for n in (1, 2)] == [1, 2, 1, 2]
    assert tc.load("synthetic32_LGL7")["N"] == 33 and tc.load("coupled12_LGL7")["N"] == 18
    for mode in ("Trapezoidal", "LGL3"):                   # stage 1 without LDS staging: (N|1) + (n|1) > 96
        f = tc.load(f"manyparams_3_90_{mode}")
        assert (f["N"] | 1) + (f["xv"] | 1) == 98
    f = tc.load("reentry_LGL5_offset1e3")
    tb = f["traj"][::f["K"], f["xv"]]
    assert tb[0] == 1.0e3 and 2.0e-4 < np.diff(tb).min() and np.diff(tb).max() < 4.0e-3
    for name in CASES:                                     # a block of h = 1e-4 beside one of h = 1
        f = tc.load(name)
        if name != "reentry_LGL5_offset1e3" and f["nb"] >= 2:
            h = np.abs(np.diff(f["traj"][::f["K"], f["xv"]]))
            a = int(h.argmin())
            assert abs(h[a] / 1e-4 - 1.0) < 1e-9 and max(h[max(a - 1, 0)], h[min(a + 1, h.size - 1)]) == h.max()
            assert abs(h.max() - 1.0) < 1e-9
    rev = [n for n in CASES if tc.load(n)["meta"]["reverse"]]
    assert len(rev) == 4 and all(tc.load(n)["traj"][0, tc.load(n)["xv"]] > tc.load(n)["traj"][-1, tc.load(n)["xv"]] for n in rev)


@pytest.mark.parametrize("name", CASES)
def test_every_case_contains_its_query_kinds(name):
    f = tc.load(name)
    t, times = f["traj"][:, f["xv"]], f["times"]
    tb = t[::f["K"]]
    have = set(times.tolist())
    assert set(t.tolist()) <= have                                                         # every node time, t0 and tf among them
    assert set(np.nextafter(tb, -np.inf).tolist()) <= have and set(np.nextafter(tb, np.inf).tolist()) <= have
    d = 1.0 if tb[-1] > tb[0] else -1.0
    inside = (d * times > d * tb[0]) & (d * times < d * tb[-1])
    edge = set(t.tolist()) | set(np.nextafter(tb, -np.inf).tolist()) | set(np.nextafter(tb, np.inf).tolist())
    rand = np.array([x for x in times[inside] if x not in edge])
    assert rand.size == f["meta"]["nrand"] >= (8 if f["N"] >= 18 else 24)
    e, _ = ick.find_blocks(tb, rand)
    assert np.sum(e == np.abs(np.diff(tb)).argmin()) >= 4                                  # the narrowest block has its share
    s0 = (times - tb[0]) / (tb[1] - tb[0])
    s1 = (times - tb[-2]) / (tb[-1] - tb[-2])
    for want, s, tol in ((-0.3, s0, 1e-6), (-1e-9, s0, 5e-10), (1.0 + 1e-9, s1, 5e-10), (1.2, s1, 1e-6)):
        assert np.any(np.abs(s - want) < tol), want
    assert f["outside"] == 6                                     # those four and the outer neighbours of t0 and tf
    # shuffled: neighbouring queries search different blocks
    assert f["nb"] == 1 or np.mean(np.diff(f["block"]) != 0) > (0.3 if f["nb"] == 2 else 0.5)


@pytest.mark.parametrize("name", CASES)
def test_blocks_and_outside_counts_agree_with_the_interpolation_checker(name):
    f = tc.load(name)
    e, outside = ick.find_blocks(f["traj"][::f["K"], f["xv"]], f["times"])
    assert np.array_equal(e, f["block"]) and outside == f["outside"]


@pytest.mark.parametrize("name", CASES)
def test_model_stays_inside_an_eighth_of_the_bound_and_is_exact_where_E_is_zero(oracle, name):
    f = tc.load(name)
    val, der, outside = tc.model(f, tc.rhs_of(oracle, f["meta"]["ode"]))
    assert outside == f["outside"]
    ids = np.arange(f["times"].size)
    xv = f["xv"]
    for k, got in (("val", val), ("der", der)):
        r = tc.check(got, f, ids, k)
        assert r["over"] == 0 and 8.0 * r["worst"] <= 1.0, (k, r)
        zero = f[k + "E"] == 0
        assert np.array_equal(got[zero], f[k][zero])
    # which entries have E = 0: the time's derivative, BlockConstant controls and parameters and their derivative -- and the time
    # itself at tau = t0, where s = 0 and tb0 + h 0 has no rounded term
    assert np.all(f["derE"][:, xv] == 0) and np.all(f["der"][:, xv] == 1.0) and np.all(f["valE"][:, :xv] > 0)
    assert np.array_equal(f["valE"][:, xv] == 0, f["times"] == f["traj"][0, xv])
    if f["meta"]["blocked"]:
        first = f["traj"][f["block"] * f["K"]]
        assert np.all(f["valE"][:, xv + 1:] == 0) and np.all(f["derE"][:, xv + 1:] == 0)
        assert np.array_equal(f["val"][:, xv + 1:], first[:, xv + 1:]) and not np.any(f["der"][:, xv + 1:])


def test_kappa_is_eight_times_the_measured_model_ratio_rounded_up_to_a_power_of_two():
    c = tc.load(CASES[0])["meta"]["constants"]
    assert c["factor"] == 8.0 and c["inexact"] == 0
    for k in tc.KINDS:
        assert c["kappa"][k] == tc.pow2_ceil(8.0 * c["worst"][k]) == tc.KAPPA[k], (k, c["worst"][k])
    for name in CASES:                                     # the same record in every file
        assert tc.load(name)["meta"]["constants"] == c


def test_generator_reproduces_a_stored_file_bit_for_bit(gen):
    name = "reentry_LGL7_nb1"
    c = gen.case_by_name(name)
    buf = io.BytesIO()
    gen.write_npz(buf, dict(gen.compute_case(c), meta=gen.meta_of(c, tc.load(name)["meta"]["constants"])))
    assert buf.getvalue() == open(os.path.join(tc.DIR, name + ".npz"), "rb").read()


def test_check_counts_every_entry_a_nan_and_a_change_where_E_is_zero():
    f = tc.load("twobody_lt_LGL5_blocked")
    ids = np.arange(f["times"].size)
    assert tc.check(f["val"], f, ids, "val") == dict(worst=0.0, where=(0, 0), over=0, n=f["val"].size)
    sub = np.array([5, 3, 3, 40])
    assert tc.check(f["der"][sub], f, sub, "der")["n"] == 4 * f["N"]
    v = f["val"].copy()
    v[7, 2] *= 1.0 + 1e-11                                  # far inside the old tolerance of 1e-10
    assert tc.check(v, f, ids, "val")["over"] == 1
    v = f["val"].copy()
    v[9, f["xv"] + 1] = np.nextafter(v[9, f["xv"] + 1], np.inf)
    r = tc.check(v, f, ids, "val")
    assert r["over"] == 1 and r["worst"] == np.inf and r["where"] == (9, f["xv"] + 1)
    v[9, f["xv"] + 1] = np.nan
    assert tc.check(v, f, ids, "val")["over"] == 1


# --------------------------------------------------------------------------- the fixture has teeth
def _mutated(oracle, name, **mutation):
    f = tc.load(name)
    val, der, outside = tc.model(f, tc.rhs_of(oracle, f["meta"]["ode"]), **mutation)
    ids = np.arange(f["times"].size)
    out = {}
    for k, got in (("val", val), ("der", der)):
        r = tc.check(got, f, ids, k)
        q, col = r["where"]
        print(f"[traj table] {name} {mutation}: {k} {r['over']} of {r['n']} entries over the bound, worst {r['worst']:.3g} x at query {q} "
              f"(tau = {f['times'][q]!r}, block {f['block'][q]}) column {col}")
        with np.errstate(divide="ignore", invalid="ignore"):
            out[k] = ~(np.abs(got - f[k]) <= tc.bound(f[k + "E"], k))
    return f, out, outside


@pytest.mark.parametrize("name", ["reentry_LGL7", "twobody_lt_LGL7", "synthetic32_LGL7", "brachistochrone_LGL7_nodes64"])
def test_mutation_plain_double_horner_fails_on_the_narrow_blocks_derivatives(oracle, name):
    f, over, _ = _mutated(oracle, name, horner="plain")
    narrow = f["block"] == np.abs(np.diff(f["traj"][::f["K"], f["xv"]])).argmin()
    assert over["der"][narrow][:, :f["xv"]].any(), "no derivative entry of the narrow block is over its bound"
    assert over["val"].any()                               # (and values beside a node, where a basis function is ~1e-12)


def test_mutation_boundary_time_given_to_the_block_that_starts_there(oracle):
    f, over, _ = _mutated(oracle, "twobody_lt_LGL5_blocked", boundary="start")       # BlockConstant controls of the wrong block
    tb = f["traj"][::f["K"], f["xv"]]
    at = np.isin(f["times"], tb[1:-1])
    assert at.sum() == f["nb"] - 1 and over["val"][at][:, f["xv"] + 1:].all() and not over["val"][~at].any()
    f, over, _ = _mutated(oracle, "reentry_LGL5", boundary="start")                  # the control polynomial's slope of the wrong block
    at = np.isin(f["times"], f["traj"][::f["K"], f["xv"]][1:-1])
    assert over["der"][at][:, f["xv"] + 1:].all() and not over["der"][~at].any()


def test_mutation_block_constant_controls_from_the_blocks_last_row(oracle):
    f, over, _ = _mutated(oracle, "vanderpol_LGL7_blocked", blocked_row="last")
    assert over["val"][:, f["xv"] + 1].all() and not over["val"][:, :f["xv"] + 1].any()    # (the parameter is the same in every row)


@pytest.mark.parametrize("name,k", [("brachistochrone_Trapezoidal_nodes65", 64), ("brachistochrone_LGL5_nodes65", 32)])
def test_mutation_last_block_time_of_a_65_node_mesh_left_at_zero(oracle, name, k):
    f, over, outside = _mutated(oracle, name, tb_zero=k)
    assert f["traj"].shape[0] == 65 and k == f["nb"]       # the entry the lone thread of the second stage-1 workgroup stores
    assert over["val"].any() and over["der"].any() and outside != f["outside"]


def test_mutation_time_reversed_search_run_forward(oracle):
    f, over, outside = _mutated(oracle, "reentry_LGL7_reversed", direction=1.0)
    assert over["val"].any() and over["der"].any() and outside != f["outside"]
