"""CPU tests of the KKT-map builder (csrc/capi/kkt_map.h: build_kkt_map) through asset_hip_kkt_map_query -- no handle, no device.

tests/golden/kkt_map/kkt_maps.npz holds what asset_hip_defect_set_kkt_map computed on the host BEFORE that arithmetic became a function
of its own: it was recorded (tests/golden/kkt_map/record.py) from a build in which build_kkt_map was the entry point's text moved
verbatim -- `h->ke->ir`, `h->ke->orr`, `h->ke->nkkt`, `h->ke->mode == ASSET_HIP_FUNCTION` and `h->nseg` replaced by parameters, nothing else
-- and only tidied afterwards.  Every map word, both reduction lists and the value range are stored by value (the long arrays as first
differences, `x.diff`: their running sum is x).  The inputs are the locations the oracle's sparsity analysis gives, as
tests/test_gpu_assembly.py:_setup asks for them, at small meshes; they are stored too, so that a change of the oracle's numbering
reads as that and not as a change of the builder."""
import os

import numpy as np
import pytest

from asset_asrl_amd import _lib
from helpers import Workload

FIX = os.path.join(os.path.dirname(__file__), "golden", "kkt_map", "kkt_maps.npz")

# name: (ode, mode, nseg, blocked, plain_function, accumulate, drop the Jacobian slots)
CASES = {
    "reentry_lgl7": ("reentry", "LGL7", 6, False, False, False, False),                 # two row tiles; boundary nodes shared by neighbours
    "twobody_lt_lgl5_blocked": ("twobody_lt", "LGL5", 7, True, False, False, False),    # BlockConstant: per-segment control parameters
    "betts_lgl5": ("betts_lowthrust", "LGL5", 9, False, False, False, False),           # a phase parameter every segment shares: staged
    "brachistochrone_trap": ("brachistochrone", "Trapezoidal", 8, False, False, False, False),
    "synthetic32_lgl7": ("synthetic32", "LGL7", 3, False, False, False, False),         # the wide shape
    "plain_function": ("brachistochrone", "Trapezoidal", 8, False, True, False, False),  # entries slot by slot, no fragment order
    "reentry_lgl7_accumulate": ("reentry", "LGL7", 6, False, False, True, False),       # every slot an atomic add
    "betts_lgl5_hessian_only": ("betts_lowthrust", "LGL5", 9, False, False, False, True),   # -1 slots (an objective keeps no Jacobian slot)
}


def case_inputs(oracle, name):
    """(IR, OR, plain_function, accumulate, slot_locations[nseg, NKKT], nvalues) of a case."""
    ode, mode, nseg, blocked, plain, accumulate, hessian_only = CASES[name]
    w = Workload(ode, mode, nseg, blocked, var_offset=3, con_offset=2, extra_vars=4)
    nlp = w.oracle_nlp(oracle, threads=2)
    locs = nlp.kkt_locations()[:nlp.num_user_kkt].reshape(w.nseg, w.NKKT).astype(np.int32)
    if hessian_only:          # the reference's slot order: per block column c, (IR - c) Hessian slots, then OR Jacobian slots
        k = 0
        for c in range(w.IR):
            k += w.IR - c
            locs[:, k:k + w.OR] = -1
            k += w.OR
    return w.IR, w.OR, plain, accumulate, locs, int(nlp.nnz)


def kinds_of(words, nvalues):
    """How many map words store, add atomically, write a staging cell, drop."""
    w = words.astype(np.int64)
    return {"stored": int((w >= 0).sum()), "added": int(((w <= -2) & (-w - 2 < nvalues)).sum()),
            "staged": int((-w - 2 >= nvalues).sum()), "dropped": int((w == -1).sum())}


@pytest.fixture(scope="module")
def recorded():
    z = np.load(FIX)
    assert sorted(str(n) for n in z["cases"]) == sorted(CASES)
    rec = {}
    for k in z.files:
        rec[k[:-5] if k.endswith(".diff") else k] = np.cumsum(z[k]).astype(np.int32) if k.endswith(".diff") else z[k]
    for n in CASES:
        rec[n + "/slot_locations"] = rec[n + "/slot_locations"].reshape(int(rec[n + "/nseg"]), -1)
    return rec


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_recorded_map_is_reproduced(oracle, recorded, name):
    z = recorded
    ir, orr, plain, accumulate, locs, nvalues = case_inputs(oracle, name)
    np.testing.assert_array_equal(locs, z[name + "/slot_locations"])      # (the oracle's numbering, not the builder, when this fails)
    assert nvalues == int(z[name + "/nvalues"])
    words, ptr, loc, lo, hi = _lib.kkt_map(ir, orr, plain, locs, nvalues, accumulate)
    np.testing.assert_array_equal(words, z[name + "/map_words"])
    np.testing.assert_array_equal(ptr, z[name + "/multi_ptr"])
    np.testing.assert_array_equal(loc, z[name + "/multi_loc"])
    assert (lo, hi) == tuple(z[name + "/range"].tolist())
    assert words.size == (locs.size if plain else locs.shape[0] * _fragment_words(ir, orr))


def _fragment_words(ir, orr):
    ti, tj = (ir + 15) // 16, (orr + 15) // 16
    return (ti * (ti + 1) // 2 + ti * tj) * 4 * 64


def test_the_recording_holds_every_encoding(recorded):
    """Not vacuous: stores, atomic adds and staged cells all occur, and where they must."""
    z = recorded
    k = {n: kinds_of(z[n + "/map_words"], int(z[n + "/nvalues"])) for n in CASES}
    for n in ("reentry_lgl7", "twobody_lt_lgl5_blocked", "betts_lgl5", "brachistochrone_trap", "synthetic32_lgl7", "plain_function"):
        assert k[n]["stored"] > 0 and k[n]["added"] > 0, (n, k[n])         # interior entries; the node two neighbours share
    assert z["reentry_lgl7/multi_loc"].size == 0 and k["reentry_lgl7"]["staged"] == 0     # no location has a third contributor
    for n in ("betts_lgl5", "betts_lgl5_hessian_only"):                    # the phase parameter: one contribution per segment
        nseg = CASES[n][2]
        ptr = z[n + "/multi_ptr"]
        assert z[n + "/multi_loc"].size > 0 and np.diff(ptr).max() == nseg and k[n]["staged"] == ptr[-1]
        assert np.all(np.diff(z[n + "/multi_loc"]) > 0)
    a = k["reentry_lgl7_accumulate"]
    assert a["stored"] == 0 and a["staged"] == 0 and a["added"] == k["reentry_lgl7"]["stored"] + k["reentry_lgl7"]["added"]
    assert k["betts_lgl5_hessian_only"]["dropped"] > k["betts_lgl5"]["dropped"]
    # a plain function's map is the slot order itself: one word per slot
    assert z["plain_function/map_words"].size == z["plain_function/slot_locations"].size
    assert k["plain_function"]["dropped"] == 0 and k["brachistochrone_trap"]["dropped"] > 0    # (padding of the fragments)


def test_kkt_map_query_refusals(oracle):
    ir, orr, _, _, locs, nvalues = case_inputs(oracle, "betts_lgl5")
    bad = locs.copy()
    bad[3, 5] = nvalues
    with pytest.raises(_lib.AssetHipError, match=r"rc=-4\).*outside \[0, nvalues\)"):
        _lib.kkt_map(ir, orr, False, bad, nvalues)
    bad[3, 5] = -2
    with pytest.raises(_lib.AssetHipError, match="outside"):
        _lib.kkt_map(ir, orr, False, bad, nvalues)
    with pytest.raises(_lib.AssetHipError, match="keeps no slot"):
        _lib.kkt_map(ir, orr, False, np.full_like(locs, -1), nvalues)
    cells = 9                                                              # one staged location, a cell per segment
    fits = 2**31 - 1 - 2 - cells                                           # value array + staging cells + 2 <= INT32_MAX
    assert _lib.kkt_map(ir, orr, False, locs, fits)[1][-1] == cells
    with pytest.raises(_lib.AssetHipError, match=r"rc=-4\).*exceed the 32-bit map range"):
        _lib.kkt_map(ir, orr, False, locs, fits + 1)
    _lib.kkt_map(ir, orr, False, locs, fits + 1, accumulate=True)          # (no staging in accumulate mode: nothing to overflow)
    with pytest.raises(_lib.AssetHipError, match="bad kkt map arguments"):
        _lib.kkt_map(ir, orr, False, locs, 0)
    # a Jacobian slot at a location that is staged for its Hessian slots: the reduction ASSIGNS the staged sum, the add would be lost
    staged_loc = _lib.kkt_map(ir, orr, False, locs, nvalues)[2][0]
    bad = locs.copy()
    bad[2, ir] = staged_loc                                                # (slot IR of a block: J(0, 0), behind the IR Hessian slots of column 0)
    with pytest.raises(_lib.AssetHipError, match=r"rc=-1\).*Jacobian slot names a location that is staged"):
        _lib.kkt_map(ir, orr, False, bad, nvalues)
    _lib.kkt_map(ir, orr, False, bad, nvalues, accumulate=True)            # (every slot an add: nothing is assigned)
