"""Every entry the device trajectory table writes (asset_asrl_amd/interp.py -> asset_hip_traj_table_* -> csrc/interp_kernels.h), values
and time derivatives, against 50 digits with a bound per entry (tests/traj_table_checker.py; fixtures: tests/golden/traj_table/, made
by tests/golden/make_golden_traj_table.py).

* every case of the fixture, every entry: every mode forward and time-reversed, BlockConstant, rows of 33 and 94 columns (the latter
  through stage 1's branch without LDS staging), one and two blocks, node counts either side of a stage-1 workgroup, times near 1e3
  with h ~ 1e-3, blocks of h = 1e-4 beside blocks of h = 1; queries at every node, on both sides of every block boundary, outside;
* query counts either side of a stage-2 workgroup of 128;
* the grid-stride loop of stage 2, by tiling: query j of a run of (8 CUs + 1) 128 + 1 is fixture query pi(j) -- a fixed pseudo-random
  map in which no two neighbours are equal -- and every entry of every row is checked.

The worst |got - ref| / bound of every case is printed (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

import traj_table_checker as tc
from asset_asrl_amd import _lib
from asset_asrl_amd.interp import LGLInterpTable
from test_gpu_defect_entries import device_cus, tiling

pytestmark = pytest.mark.gpu

CASES = tc.all_cases()
NARROW, WIDE = "brachistochrone_LGL7_nodes64", "synthetic32_LGL7"


def device_ode(name: str):
    """What LGLInterpTable is handed for a fixture's ODE: a library ODE's name, a run-time compiled one's definition"""
    import helpers
    made = {"vanderpol": helpers.make_vanderpol, "coupled12": helpers.make_coupled12, "manyparams_3_90": helpers.make_manyparams}
    return made[name]() if name in made else name


def table_of(f):
    m = f["meta"]
    t = LGLInterpTable(device_ode(m["ode"]), f["traj"], m["mode"], m["blocked"])
    t.WarnOutOfBounds = False
    assert (t.NumBlocks, t.T0, t.TF, t.XtUPVars) == (f["nb"], f["traj"][0, f["xv"]], f["traj"][-1, f["xv"]], f["N"])
    return t


def assert_rows(tag, f, ids, val, der):
    rv, rd = tc.check(val, f, ids, "val"), tc.check(der, f, ids, "der")
    print(f"[traj table] {tag}: worst |got - ref| / bound  val {rv['worst']:.3g}  der {rd['worst']:.3g}  ({rv['n'] + rd['n']} entries)")
    assert rv["over"] == 0 and rd["over"] == 0, (tag, rv, rd, [float(f["times"][ids[r["where"][0]]]) for r in (rv, rd)])


@pytest.mark.parametrize("name", CASES)
def test_every_case_every_entry(name):
    f = tc.load(name)
    with table_of(f) as table:
        val, der = table.InterpolateDeriv(f["times"])
        assert table.last_outside == f["outside"]
        only = table.Interpolate(f["times"])
        assert table.last_outside == f["outside"]
    assert_rows(name, f, np.arange(f["times"].size), val, der)
    assert np.array_equal(only, val)                       # with and without the derivative output: the same values, bit for bit


@pytest.mark.parametrize("n", [1, 127, 128, 129])
@pytest.mark.parametrize("name", [NARROW, WIDE])
def test_query_counts_either_side_of_a_workgroup(name, n):
    f = tc.load(name)
    assert f["times"].size >= 129
    ids = np.arange(n)
    d = 1.0 if f["traj"][-1, f["xv"]] > f["traj"][0, f["xv"]] else -1.0
    t = f["times"][:n]
    with table_of(f) as table:
        val, der = table.InterpolateDeriv(t)
        assert table.last_outside == int(np.sum((d * t < d * table.T0) | (d * t > d * table.TF)))
    assert val.shape == der.shape == (n, f["N"])
    assert_rows(f"{name} first {n}", f, ids, val, der)


@pytest.mark.parametrize("name", [NARROW, WIDE])
def test_grid_stride_loop_by_tiling(name):
    import torch
    f = tc.load(name)
    cus = device_cus()
    nq = (8 * cus + 1) * 128 + 1
    groups, grid = (nq + 127) // 128, 8 * cus
    pi = tiling(nq, f["times"].size)
    assert np.all(pi[1:] != pi[:-1]) and np.unique(pi).size == f["times"].size
    d = 1.0 if f["traj"][-1, f["xv"]] > f["traj"][0, f["xv"]] else -1.0
    out_of = (d * f["times"] < d * f["traj"][0, f["xv"]]) | (d * f["times"] > d * f["traj"][-1, f["xv"]])
    assert int(out_of.sum()) == f["outside"]
    want_outside = int(out_of[pi].sum())
    L = _lib.lib()
    d_t = torch.from_numpy(f["times"][pi]).cuda()
    with table_of(f) as table:
        assert table._h is not None
        for counted in (True, False):
            d_out = torch.full((nq, f["N"]), float("nan"), dtype=torch.float64, device="cuda")
            d_dout = torch.full((nq, f["N"]), float("nan"), dtype=torch.float64, device="cuda")
            d_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            _lib.check(L.asset_hip_traj_table_interp_device(table.handle, C.c_void_p(d_t.data_ptr()), nq, 1, C.c_void_p(d_out.data_ptr()),
                                                            C.c_void_p(d_dout.data_ptr()),
                                                            C.c_void_p(d_cnt.data_ptr()) if counted else None, None),
                       "asset_hip_traj_table_interp_device")
            torch.cuda.synchronize()
            assert int(d_cnt.item()) == (want_outside if counted else 0)
            assert_rows(f"{name} tiled x{nq} ({groups} groups of 128 on a grid of {grid}; counter {'on' if counted else 'null'})",
                        f, pi, d_out.cpu().numpy(), d_dout.cpu().numpy())
    assert groups > grid                                    # the loop did run: more groups than workgroups
