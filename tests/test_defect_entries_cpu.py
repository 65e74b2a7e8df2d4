"""CPU tests of the per-entry defect fixtures (tests/golden/defect_entries/, tests/defect_checker.py): the oracle -- both derivative
providers -- stays inside the bound on every entry of every fixture, with the factor 8 the device is given to spare (that is where the
four kappa come from); the fixtures agree with the 11 old golden vectors; the generator reproduces a stored segment bit for bit; the
running-error rules give the textbook answers on a sum and a Horner polynomial."""
import glob
import os
import sys

import numpy as np
import pytest

import defect_checker as dc

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SHAPES = dc.all_shapes()
IDS = [dc.shape_name(*s) for s in SHAPES]


@pytest.fixture(scope="module")
def gen():
    sys.path.insert(0, GOLDEN)
    import make_golden_defect_entries as g
    return g


def test_fixture_covers_every_library_shape_and_the_run_time_families(gen):
    from asset_asrl_amd import _lib
    lib = [(o, m, b) for o in ("brachistochrone", "reentry", "twobody_lt", "betts_lowthrust", "synthetic32")
           for m in ("Trapezoidal", "LGL3", "LGL5", "LGL7") for b in (False, True) if _lib.has_kernel(o, _lib.MODES[m], b)]
    assert len(lib) == 36 and set(lib) <= set(SHAPES)
    assert sorted(SHAPES) == sorted(gen.shapes())
    extra = set(SHAPES) - set(lib)
    assert extra == {("coupled12", "LGL7", False), ("driven14", "LGL7", False), ("shape_1_0_0", "LGL5", False),
                     ("shape_2_13_0", "LGL5", False), ("shape_2_13_0", "LGL5", True), ("shape_5_3_2", "LGL5", False),
                     ("shape_5_3_2", "LGL5", True)}
    limit = os.path.getsize(os.path.join(GOLDEN, "mesh_error.npz"))
    for s in SHAPES:
        f = dc.load(s)
        assert os.path.getsize(os.path.join(dc.DIR, dc.shape_name(*s) + ".npz")) <= limit
        assert f["x"].shape[0] == (2 if s[0] in gen.WIDE else 6)
        assert f["meta"]["flags"] == [fl for _, fl in gen.segment_plan(*s)[2]]
        for k in dc.KINDS:
            assert f[k].dtype == np.float64 and f[k + "E"].dtype == np.float32 and f[k].shape == f[k + "E"].shape
            assert np.all(np.isfinite(f[k])) and np.all(np.isfinite(f[k + "E"])) and np.all(f[k + "E"] >= 0)
        assert f["hx"].shape[1] == f["IR"] * (f["IR"] + 1) // 2
        # the edges the segments are there for
        for x, lam, fl in zip(f["x"], f["lam"], f["meta"]["flags"]):
            xv, uv, pv = f["meta"]["sizes"]
            q = xv + 1 + (0 if s[2] else uv)
            h = x[(f["IR"] - pv - (uv if s[2] else 0)) - q + xv] - x[xv]
            assert (h < 0) == bool(fl & gen.REVERSED) and (abs(h) < 1e-3) == bool(fl & gen.NARROW)
            if fl & gen.WIDELAM:
                assert np.abs(lam).max() == 1e3 and np.sum(lam == 0) == min(2, max(1, lam.size - 2))
                assert lam.size == 2 or np.abs(lam[lam != 0]).min() == 1e-6


@pytest.mark.parametrize("shape,provider", [(s, p) for s in SHAPES for p, _ in dc.providers(s[0])],
                         ids=[f"{dc.shape_name(*s)}-{n}" for s in SHAPES for _, n in dc.providers(s[0])])
def test_oracle_stays_inside_an_eighth_of_the_bound(oracle, shape, provider):
    """The proof that the reference alone is inside the bound, and that kappa is what defect_checker says it is: 8 x the oracle's worst
    ratio does not exceed it.  Entries with E = 0 are reproduced exactly."""
    f = dc.load(shape)
    got = dc.oracle_blocks(oracle, f, provider)
    ids = np.arange(f["x"].shape[0])
    for k in dc.KINDS:
        r = dc.check(got[k], f, ids, k)
        assert r["over"] == 0 and 8.0 * r["worst"] <= 1.0, (k, r)
        zero = f[k + "E"] == 0
        assert np.array_equal(got[k].reshape(f[k].shape)[zero], f[k][zero])


def test_kappa_is_eight_times_the_measured_oracle_ratio_rounded_up_to_a_power_of_two():
    c = dc.load(SHAPES[0])["meta"]["constants"]
    assert c["factor"] == 8.0 and c["inexact"] == 0
    for k in dc.KINDS:
        w = max(c["worst"][k].values())
        assert c["kappa"][k] == dc.pow2_ceil(8.0 * w) == dc.KAPPA[k], (k, w)
    for s in SHAPES:                                       # the same record in every file
        assert dc.load(s)["meta"]["constants"] == c


OLD = sorted(p for p in glob.glob(os.path.join(GOLDEN, "*.npz"))
             if os.path.basename(p) not in ("pathfuncs.npz", "vf_ops.npz", "mesh_error.npz"))


@pytest.mark.parametrize("path", OLD, ids=[os.path.basename(p)[:-4] for p in OLD])
def test_fixture_equals_the_old_golden_vector_where_segments_coincide(path):
    g = np.load(path)
    f = dc.load((str(g["ode"]), str(g["mode"]), bool(g["blocked"])))
    assert f["meta"]["seed"] == int(g["seed"]) and f["meta"]["mesh_segments"] == int(g["mesh_segments"])
    il = np.tril_indices(f["IR"])
    hit = 0
    for i, seg in enumerate(g["segments"].tolist()):
        k = [j for j, (s, fl) in enumerate(zip(f["meta"]["segments"], f["meta"]["flags"])) if s == seg and fl == 1]
        assert len(k) == 1
        k = k[0]
        hit += 1
        assert np.array_equal(f["x"][k], g["x"][i]) and np.array_equal(f["lam"][k], g["lam"][i])
        for a, b in ((f["fx"][k], g["fx"][i]), (f["jx"][k], g["jx"][i]), (f["gx"][k], g["gx"][i]), (f["hx"][k], g["hx"][i][il])):
            assert np.all(np.abs(a - b) <= 2.0 ** -52 * np.abs(b))          # both are a 50-digit value rounded to float64
    assert hit == len(g["segments"])


def test_generator_reproduces_a_stored_segment_bit_for_bit(gen):
    shape, k = ("brachistochrone", "LGL3", False), 3          # the narrow segment of the smallest shape
    f = dc.load(shape)
    assert f["meta"]["flags"][k] == gen.NARROW
    s = gen.compute_segment(*shape, k)
    for key, a in s.items():
        assert a.dtype == f[key].dtype and np.array_equal(a, f[key][k]), key


def test_running_error_of_a_sum_is_the_sum_of_its_partial_sums(gen):
    """Recursive summation s_k = s_{k-1} + x_k: the running bound is sum_{k >= 2} |s_k| (Higham, section 4.3), inside the a priori bound
    (n - 1) sum |x_i|; the float64 sum is inside u E."""
    import mpmath as mp
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, 40)
    v = [gen.DE.var(mp.mpf(float(t)), i, x.size) for i, t in enumerate(x)]
    acc = 0
    for t in v:
        acc = acc + t
    part = np.cumsum([mp.mpf(float(t)) for t in x])
    want = float(sum(abs(p) for p in part[1:]))
    assert abs(acc.ev - want) <= 1e-12 * want and acc.ev <= (x.size - 1) * np.abs(x).sum()
    assert np.all(acc.eg == 0) and np.all(acc.eh == 0)                    # 0 + 1 and 0 + 0: no rounded term
    fl = 0.0
    for t in x:
        fl += float(t)
    assert abs(mp.mpf(fl) - acc.v) <= dc.U * acc.ev
    ones = [gen.DE.var(mp.mpf(1), i, 5) for i in range(5)]
    assert (ones[0] + ones[1] + ones[2] + ones[3] + ones[4]).ev == 2 + 3 + 4 + 5


def test_running_error_of_a_horner_polynomial_is_highams(gen):
    """Horner's rule p = p x + a_i: Higham's running bound (Algorithm 5.1: mu = mu |x| + |p| per step, here counted per operation:
    |p x| for the product, |p x + a| for the sum), inside the a priori bound 2 n sum |a_i| |x|^i; the derivative's bound follows the
    product rule term by term; the float64 evaluation is inside u E."""
    import mpmath as mp
    a = [0.3, -1.7, 2.9, 0.11, -4.3, 1.9, 0.7]
    x0 = 0.83
    x = gen.DE.var(mp.mpf(x0), 0, 1)
    p = gen.DE.const(a[0], 1)
    pv, e = mp.mpf(a[0]), 0.0
    dv, de = mp.mpf(0), 0.0                                                # the derivative recurrence p' = p' x + p
    for c in a[1:]:
        t1 = dv * mp.mpf(x0)
        et1 = abs(x0) * de + (float(abs(t1)) if dv != 0 else 0.0)
        et2 = e + float(abs(pv))                                           # (x' p = 1 p is counted as a product)
        nd = t1 + pv
        de = et1 + et2 + (float(abs(nd)) if t1 != 0 else 0.0)
        dv = nd
        t = pv * mp.mpf(x0)
        e = abs(x0) * e + float(abs(t))
        pv = t + mp.mpf(c)
        e = e + float(abs(pv))
        p = p * x + c
    n = len(a) - 1
    assert p.v == pv and abs(p.ev - e) <= 1e-12 * e
    assert p.ev <= 2 * n * sum(abs(c) * abs(x0) ** (n - i) for i, c in enumerate(a))
    assert p.g[0] == dv and abs(p.eg[0] - de) <= 1e-12 * de
    fl = a[0]
    for c in a[1:]:
        fl = fl * x0 + c
    assert abs(mp.mpf(fl) - p.v) <= dc.U * p.ev


def test_check_sees_what_the_old_tolerance_does_not():
    """The checker itself: a small entry set to zero, a last-digit change and a non-zero at a structural zero are all over the bound,
    the untouched reference is not."""
    f = dc.load(("reentry", "LGL7", False))
    ids = np.arange(f["x"].shape[0])
    assert dc.check(f["hx"], f, ids, "hx") == dict(worst=0.0, where=(0, 0), over=0, n=f["hx"].size)
    h = f["hx"].copy()
    small = (np.abs(h) < 1e-9 * np.abs(h).max(axis=1, keepdims=True)) & (h != 0)
    assert small.sum() > 0
    h[small] = 0.0
    assert dc.check(h, f, ids, "hx")["over"] == small.sum()
    j = f["jx"].copy()
    at = np.unravel_index(np.abs(j).argmax(), j.shape)
    j[at] *= 1.0 + 1e-11
    assert dc.check(j, f, ids, "jx")["over"] == 1
    z = np.argwhere(f["hxE"] == 0)
    assert len(z) > 0
    h = f["hx"].copy()
    h[tuple(z[0])] = 1e-300
    r = dc.check(h, f, ids, "hx")
    assert r["over"] == 1 and r["worst"] == np.inf and r["where"] == tuple(z[0])
    h[tuple(z[0])] = np.nan
    assert dc.check(h, f, ids, "hx")["over"] == 1
