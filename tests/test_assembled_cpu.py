"""CPU tests of tests/assembled_checker.py -- the per-location checker of the on-device KKT assembly -- and of the maps it constructs,
through asset_hip_kkt_map_query (no handle, no device):

* the restated reductions against math.fsum;
* every constructed map the GPU tests set (assembled_checker.CONSTRUCTED) comes back from build_kkt_map with the classes, the
  encodings, the staging lists and the range it was constructed with;
* the per-location bound is not vacuous and not too tight: the oracle's blocks (both derivative providers), scattered through every
  map sequentially in three random orders, use at most half of it at every location (pytest -s prints the worst ratio per shape);
* build_kkt_map refuses a Jacobian slot at a location staged for Hessian slots."""
import math

import numpy as np
import pytest

import assembled_checker as ac
import defect_checker as dc
from asset_asrl_amd import _lib
from test_kkt_map_cpu import kinds_of

SIZES = (1, 2, 3, 64, 65, 255, 256, 257, 512, 513)
IDS = [ac.constructed_id(c) for c in ac.CONSTRUCTED]


def _terms(k, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, k) * 10.0 ** rng.integers(-6, 3, k)
    if k >= 3:                                             # cancelling terms: the sum is far below sum |c|
        c[1::2][:k // 2] = -c[0::2][:k // 2] * (1.0 + rng.uniform(-1e-9, 1e-9, k // 2))
    return c


@pytest.mark.parametrize("k", SIZES)
def test_restated_reductions_against_fsum(k):
    for seed in range(4):
        c = _terms(k, 100 * k + seed)
        exact, tol = math.fsum(c), (k - 1) * ac.U * math.fsum(np.abs(c))
        assert abs(ac.reduce_staged(c) - exact) <= tol
        base = float(np.random.default_rng(seed).uniform(-1, 1))
        for g in (ac.gather_short, ac.gather_long):        # one more addition: the base
            got = g(base, c)
            assert abs(got - math.fsum([base, *c])) <= tol + ac.U * abs(got)
    if k == 1:
        assert ac.reduce_staged(c) == c[0] and ac.gather_short(0.0, c) == c[0] and ac.gather_long(0.0, c) == c[0]


def test_restated_reductions_follow_the_kernels_order():
    """Sums in which the order shows: 2^53 absorbs a 1 that is added to it alone."""
    big = 2.0 ** 53
    assert ac.gather_short(0.0, [big, 1.0, 1.0, -big]) == 0.0 and ac.gather_short(0.0, [1.0, 1.0, big, -big]) == 2.0
    c = np.zeros(513)
    c[0], c[256], c[512] = big, 1.0, 1.0                   # all three are thread 0's cells: (big + 1) + 1 = big
    assert ac.reduce_staged(c) == big
    c = np.zeros(513)
    c[0], c[1], c[257] = big, 1.0, 1.0                     # thread 1 adds its two first, the tree folds 2 into thread 0's
    assert ac.reduce_staged(c) == big + 2.0
    c = np.zeros(257)
    c[0], c[128], c[256] = big, 1.0, -big                  # thread 0: big - big = 0, then the tree's first step brings in cell 128
    assert ac.reduce_staged(c) == 1.0 and ac.gather_long(3.0, c) == 4.0
    c[128], c[255] = 0.0, 1.0                              # a stride of 255 would hand cell 255 to thread 0 between the two
    assert ac.reduce_staged(c) == 1.0
    # the split: 64 contributors are a short row, 65 a long one
    t = np.zeros(65)
    t[0], t[1], t[3] = big, 1.0, 1.0                       # (long: threads 1 and 3 meet in the tree before they reach thread 0)
    out, n = ac.gather(np.r_[np.zeros(64, int), np.ones(65, int)], np.r_[t[:64], t], np.zeros(2))
    assert n.tolist() == [64, 65] and out.tolist() == [big, big + 2.0]


@pytest.mark.parametrize("case", ac.CONSTRUCTED, ids=IDS)
def test_constructed_map_comes_back_as_constructed(case):
    shape, nseg, spec, _ = case
    f = dc.load(shape)
    IR, OR = f["IR"], f["OR"]
    locs, nvalues = ac.constructed_map(case)
    want = ac.intended(nseg, IR, OR, spec)
    has = ac.classes_of(locs, IR, OR)
    assert has["mixed"] == 0 and has["dropped"] == want["dropped"]
    assert has["hess"][has["hess"] > 1].tolist() == want["hess"]
    assert has["jac"][has["jac"] > 1].tolist() == [s for s in want["jac"] if s > 1]
    words, ptr, loc, lo, hi = _lib.kkt_map(IR, OR, False, locs, nvalues)
    k = kinds_of(words, nvalues)
    kept = locs.size - want["dropped"]
    assert (k["stored"], k["added"], k["staged"]) == (want["stored"], want["added"], want["staged"]), (k, want)
    assert k["dropped"] == words.size - kept               # the dropped slots and the padding of the fragments
    assert sorted(np.diff(ptr).tolist()) == want["staged_sizes"] and ptr[-1] == want["staged"]
    assert (lo, hi) == (want["lo"], want["hi"]) and hi <= nvalues
    if "lo" in spec:
        assert lo >= 11
    # the staged locations are the Hessian classes of three or more, in ascending order
    flat = locs.ravel()
    big = np.unique(flat[flat >= 0][np.bincount(flat[flat >= 0])[flat[flat >= 0]] >= 3])
    is_h = np.tile(ac.hessian_slots(IR, OR), nseg)
    hbig = np.asarray([m for m in big if is_h[flat == m].all()], dtype=np.int32)
    np.testing.assert_array_equal(loc, hbig)
    # every staging cell is handed out exactly once, and the cells of a location go to its slots in slot order (a plain function's map
    # is the encoding slot by slot; the fragment order holds the same words)
    enc = _lib.kkt_map(IR, OR, True, locs, nvalues)[0].astype(np.int64)
    assert np.array_equal(np.sort(enc[enc != -1]), np.sort(words.astype(np.int64)[words != -1]))
    cell = -enc - 2 - nvalues
    assert np.array_equal(np.sort(cell[cell >= 0]), np.arange(ptr[-1]))
    for l, m in enumerate(loc):
        assert np.array_equal(cell[flat == m], np.arange(ptr[l], ptr[l + 1])), (l, m)
    # accumulate mode: every kept slot an atomic add
    words, ptr, loc, lo2, hi2 = _lib.kkt_map(IR, OR, False, locs, nvalues, accumulate=True)
    k = kinds_of(words, nvalues)
    assert k["stored"] == 0 and k["staged"] == 0 and k["added"] == kept and loc.size == 0 and (lo2, hi2) == (lo, hi)


def test_the_constructed_maps_hold_what_the_gpu_tests_are_there_for():
    staged = {}
    for shape, nseg, spec, _ in ac.CONSTRUCTED:
        staged.setdefault((shape, nseg), ac.intended(nseg, dc.load(shape)["IR"], dc.load(shape)["OR"], spec)["staged_sizes"])
    r7 = {s for (shape, n), sizes in staged.items() if shape == ac.R7 and n in (1, 2, 7) for s in sizes}
    assert {3, 4, 255, 256, 257, 513} <= r7
    assert {256, 257, 600} <= set(staged[(ac.R7, 600)])
    for shape in (ac.R7, ac.TB5, ac.B5, ac.S7, ac.C7):
        mine = [spec for s, _, spec, _ in ac.CONSTRUCTED if s == shape]
        assert any(abs(sp.get("drop", 0.0) - 0.1) < 1e-12 for sp in mine) and any(sp.get("lo", 0) >= 11 for sp in mine), shape
    assert {(s, n) for s, n, _, _ in ac.CONSTRUCTED} >= {(ac.R7, 1), (ac.R7, 2), (ac.R7, 7), (ac.R7, 600), (ac.C7, 7)} | {
        (s, n) for s in (ac.TB5, ac.B5, ac.S7) for n in (7, 300)}


@pytest.mark.parametrize("shape", [ac.R7, ac.TB5, ac.B5, ac.S7, ac.C7], ids=lambda s: dc.shape_name(*s))
def test_the_oracle_alone_uses_at_most_half_of_the_location_bound(oracle, shape):
    from test_gpu_defect_entries import tiling
    f = dc.load(shape)
    worst = 0.0
    for case in [c for c in ac.CONSTRUCTED if c[0] == shape]:
        nseg = case[1]
        locs, nvalues = ac.constructed_map(case)
        pi = tiling(nseg, f["x"].shape[0])
        r, b = ac.fixture_blocks(f, pi)
        ref, bnd, cnt = ac.sum_reference(locs, r, b, nvalues)
        assert np.all(ref[cnt == 0] == 0) and np.all(bnd[cnt == 0] == 0)
        hslot, jslot = dc.block_slots(f["IR"], f["OR"])
        flat = locs.ravel()
        keep = np.nonzero(flat >= 0)[0]
        for prov, _ in dc.providers(shape[0]):
            got = dc.oracle_blocks(oracle, f, prov)
            blk = np.zeros((f["x"].shape[0], r.shape[1]))
            blk[:, hslot], blk[:, jslot.ravel()] = got["hx"], got["jx"].reshape(blk.shape[0], -1)
            c = blk[pi].ravel()
            for seed in range(3):
                order = np.random.default_rng(seed).permutation(keep)
                vals = np.zeros(nvalues)
                np.add.at(vals, flat[order], c[order])     # sequential float64 adds in that order
                res = ac.check_sum(vals, ref, bnd)
                assert res["over"] == 0 and 2.0 * res["worst"] <= 1.0, (ac.constructed_id(case), prov, seed, res)
                worst = max(worst, res["worst"])
    print(f"[assembled entries] {dc.shape_name(*shape)}: the oracle's worst |scatter - ref| / bound over its constructed maps {worst:.3g}")


def test_a_jacobian_slot_at_a_staged_location_is_refused():
    f = dc.load(ac.R7)
    IR, OR = f["IR"], f["OR"]
    hslot, jslot = dc.block_slots(IR, OR)
    locs, nvalues = ac.make_map(4, IR, OR, {}, 1)
    ok = locs.copy()
    ok[0, jslot[0, 0]] = ok[1, hslot[5]]                   # one Hessian and one Jacobian slot: two atomic adds, nothing staged
    assert _lib.kkt_map(IR, OR, False, ok, nvalues)[2].size == 0
    for nh in (2, 3):                                      # two Hessian slots and the Jacobian slot make three: the two are staged
        bad = locs.copy()
        bad[1:nh, hslot[7]] = bad[0, hslot[7]]
        assert _lib.kkt_map(IR, OR, False, bad, nvalues)[2].size == (nh >= 3)
        bad[3, jslot[2, 3]] = bad[0, hslot[7]]
        with pytest.raises(_lib.AssetHipError, match="Jacobian slot names a location that is staged"):
            _lib.kkt_map(IR, OR, False, bad, nvalues)
        _lib.kkt_map(IR, OR, False, bad, nvalues, accumulate=True)          # (nothing is staged in accumulate mode)


ELEVEN = {"K_RES1_ASM", "K_RES2_ASM", "K_RESL1_ASM", "K_RESL2_ASM", "K_LGL1_S2_ASM", "K_LGL2_S2_ASM", "K_LGL1_S3_ASM", "K_LGL2_S3_ASM",
          "K_WIDE1_ASM", "K_WIDE2_ASM", "K_RESD_ASM"}


def test_on_256_compute_units_the_gpu_tests_plan_all_eleven_assembly_kernels():
    """tests/test_gpu_assembled_entries.py asserts that every form it plans did run; this is the other half, from the planner alone: the
    sizes it runs -- the fixture's own segments of the library shapes, the looped forms where they start -- name all eleven."""
    from asset_asrl_amd.evaluator import JAC, JAC_ADJGRAD_HESS
    named = set()
    for shape in (s for s in dc.all_shapes() if s[0] in dc.LIBRARY_ODES):
        for what in (JAC, JAC_ADJGRAD_HESS):
            steps, _ = _lib.launch_plan(shape[0], _lib.MODES[shape[1]], shape[2], what, True, dc.load(shape)["x"].shape[0], cus=256)
            named |= {s[0] for s in steps}
    assert ELEVEN - named == {"K_RESL1_ASM", "K_RESL2_ASM"}, named
    from test_gpu_defect_entries import MAX_NSEG, planned_forms
    for kernel, what in (("K_RESL1_ASM", JAC), ("K_RESL2_ASM", JAC_ADJGRAD_HESS)):
        forms = planned_forms("reentry", "LGL3", False, 256, what=what, assembled=True)
        assert any(kernel in form and sizes[0] <= MAX_NSEG for form, sizes in forms.items()), (kernel, forms)
