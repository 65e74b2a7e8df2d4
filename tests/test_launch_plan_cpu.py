"""CPU tests of the launch planner (csrc/registry.h: plan_lgl) through asset_hip_launch_plan_query -- no handle, no device.

tests/golden/launch/launch_plans.npz holds what the launcher did BEFORE it was split into a planner and an executor: the launches it
issued (recorded with the kernel launch replaced by a recorder, on the CPU) for each of the 36 library shapes, 256 and 64 compute
units, every evaluation kind as blocks and -- the kinds with KKT entries -- assembled, at every mesh size from 1 to 200 000 (and
10^6, 4 10^6) at which the sequence of (kernel, block size) changes, at the size before it, and at sizes in between (a geometric
grid: grids and group sizes vary inside an interval).  Slots are stored by name, so the numbering may change."""
import os

import numpy as np
import pytest

from asset_asrl_amd import _lib

FIX = os.path.join(os.path.dirname(__file__), "golden", "launch", "launch_plans.npz")

STEP_FIELDS = ("slot", "grid_x", "grid_y", "block", "lds_bytes", "extra_arg", "group")


@pytest.fixture(scope="module")
def recorded():
    z = np.load(FIX)
    cols = [str(c) for c in z["columns"]]
    assert cols[:7] == ["entry", "cus", "what", "assembled", "nseg", "units_gp", "nsteps"]
    assert cols[7:] == [f"s{s}_{c}" for s in range(3) for c in STEP_FIELDS]
    return z


def test_every_recorded_launch_plan_is_reproduced(recorded):
    z = recorded
    rows = z["rows"].T
    names = [str(n) for n in z["slot_names"]]
    shapes = list(zip((str(o) for o in z["entry_ode"]), z["entry_mode"].tolist(), z["entry_blocked"].tolist()))
    assert len(shapes) == 36 and len(rows) > 30000
    L = _lib.lib()
    slot_of = {}
    slot = 0
    while L.asset_hip_kernel_slot_name(slot) is not None:
        slot_of[L.asset_hip_kernel_slot_name(slot).decode()] = slot
        slot += 1
    assert sorted(slot_of.values()) == list(range(len(slot_of))) and L.asset_hip_kernel_slot_name(-1) is None
    planned = set()
    p = _lib.LaunchPlan()
    for r in rows.tolist():
        ode, mode, blocked = shapes[r[0]]
        cus, what, assembled, nseg, units_gp, nsteps = r[1:7]
        # (a plan that names a kernel the shape's static table lacks is refused: rc != 0)
        rc = L.asset_hip_launch_plan_query(ode.encode(), mode, blocked, what, assembled, nseg, cus, p)
        assert rc == 0, (ode, mode, blocked, r[1:7], L.asset_hip_last_error())
        got = [p.nsteps, p.units_gp]
        want = [nsteps, units_gp]
        for s in range(3):
            st = p.step[s]
            got += [L.asset_hip_kernel_slot_name(st.slot).decode() if s < p.nsteps else None, st.grid_x, st.grid_y, st.block,
                    st.lds_bytes, st.extra_arg, st.group] if s < p.nsteps else [None, 0, 0, 0, 0, 0, 0]
            f = r[7 + 7 * s: 14 + 7 * s]
            want += [names[f[0]] if s < nsteps else None] + f[1:]
            if s < p.nsteps:
                planned.add(st.slot)
        assert got == want, (ode, mode, blocked, dict(cus=cus, what=what, assembled=assembled, nseg=nseg), got, want)
    # every kernel a plan names is one a run-time module of an ODE names too (bit 0), and the value-only defect kernel is gone
    for slot in planned:
        assert L.asset_hip_kernel_slot_kinds(slot) & 1, L.asset_hip_kernel_slot_name(slot)
    assert not any("LGL0" in n for n in slot_of)
    # the recording covers every family the launcher has
    assert {"K_VALUE", "K_ADJGRAD", "K_RES2", "K_RESL1_ASM", "K_RESLP", "K_RES_ALT", "K_RESD", "K_UNITS0", "K_UNITS1", "K_UNITS4",
            "K_UNITSJ", "K_ROWS2", "K_WIDE1_ASM", "K_LGL1_S1", "K_LGL2_S2", "K_LGL2_S3_ASM"} <= {n for n, s in slot_of.items() if s in planned}


def test_launch_plan_query_rejects_bad_requests():
    with pytest.raises(_lib.AssetHipError):
        _lib.launch_plan("nonexistent", _lib.LGL3, False, _lib.JAC, False, 100)
    with pytest.raises(_lib.AssetHipError):
        _lib.launch_plan("reentry", _lib.LGL7, False, _lib.CON, True, 100)          # assembled kinds produce KKT entries
    with pytest.raises(_lib.AssetHipError):
        _lib.launch_plan("reentry", _lib.LGL7, False, _lib.JAC, False, 0)
    with pytest.raises(_lib.AssetHipError):
        _lib.launch_plan("reentry", _lib.LGL7, False, 7, False, 100)
    steps, units_gp = _lib.launch_plan("reentry", _lib.LGL7, False, _lib.JAC_ADJGRAD_HESS, False, 10000)
    assert [s[0] for s in steps] == ["K_RES_ALT"] and steps[0][3] == 128 and units_gp == 0
