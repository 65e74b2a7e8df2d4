"""The trajectory table (asset_asrl_amd/interp.py, csrc/interp_kernels.h) as far as it can be checked without a GPU: the C ABI
is declared, bound and exported; the two kernels are in the cross-compiled code objects of every transcription entry and in a
module compiled at run time; argument errors are raised in Python before any device call; the query times of ``NDdistribute``
are the phase's mesh times.  The numerical checks are in test_gpu_traj_interp.py."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

from asset_asrl_amd import _lib, build, interp, jit, synth
from asset_asrl_amd.ode import ShuttleReentry
from helpers import make_vanderpol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = ["asset_hip_traj_table_create", "asset_hip_traj_table_interp", "asset_hip_traj_table_interp_device",
       "asset_hip_traj_table_info", "asset_hip_traj_table_destroy"]


def test_the_five_abi_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "asset_hip.h")).read()
    declared = set(re.findall(r"\b(asset_hip_[a-z0-9_]+)\s*\(", hdr))
    L = C.CDLL(_lib.LIB_PATH)
    for name in ABI:
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
    assert "asset_hip_traj_table_t" not in declared          # the handle typedef is no function-like spelling


def test_static_code_objects_hold_the_two_kernels_for_every_transcription_entry():
    blob = open(_lib.LIB_PATH, "rb").read()
    entries = 0
    from asset_asrl_amd.ode import ODE_LIBRARY
    for ode in ODE_LIBRARY:                                   # (the ODEs linked into the library; plugins carry their own code objects)
        sn = build._struct_name(ode)
        for mode, mid in _lib.MODES.items():
            for blocked in (False, True):
                if mode == "Function" or not _lib.has_kernel(ode, mid, blocked):
                    continue
                entries += 1
                for kern in ("interp_xdot_kernel", "interp_eval_kernel"):
                    kd = f"_ZN9asset_hip{len(kern)}{kern}I{len(sn)}{sn}Li{mid}ELb{int(blocked)}EEEvNS_10InterpArgsE.kd"
                    assert kd.encode() in blob, kd            # the kernel descriptor: device code, not only a host stub
    assert entries >= 20


def test_a_run_time_compiled_module_holds_the_two_kernels(monkeypatch):
    monkeypatch.delenv("ASSET_HIP_JIT", raising=False)
    ode = make_vanderpol()
    for mode, blocked, tag in (("LGL7", True, "lgl7_1"), ("Trapezoidal", False, "trapezoidal_0")):
        name = jit.ensure_kernel(ode, mode, blocked, compile_only=True)        # compile-only, as build() uses it: no device
        mods = glob.glob(os.path.join(jit.JIT_DIR, name, f"module_{tag}_*.rtc"))
        assert len(mods) == 1
        raw = open(mods[0], "rb").read()
        n = int(raw.split(b"\n", 2)[1])
        lines = raw.split(b"\n", 2 + n)[2:2 + n]
        for kern in (b"interp_xdot_kernel", b"interp_eval_kernel"):
            lowered = [ln.split(b" ", 1)[1] for ln in lines if kern in ln]
            assert len(lowered) == 1 and lowered[0] + b".kd" in raw, kern


def test_set_traj_interpolation_defaults_to_linear_and_rejects_unknown_names():
    ph = ShuttleReentry().phase("LGL5")
    assert ph.TrajInterpolation == "linear"
    ph.setTrajInterpolation("transcription")
    assert ph.TrajInterpolation == "transcription"
    ph.setTrajInterpolation("linear")
    for bad in ("cubic", "Transcription", "", None):
        with pytest.raises(ValueError):
            ph.setTrajInterpolation(bad)
    assert ph.TrajInterpolation == "linear"


def test_default_refine_is_np_interp_bit_for_bit():
    traj = synth.make_traj("reentry", "LGL7", 9, seed=5)
    ph = ShuttleReentry().phase("LGL7", traj, 9)
    before = ph.ActiveTraj.copy()
    bins = np.array([0.0, 0.2, 0.55, 1.0])
    ph.refineTrajManual(bins, [3, 2, 4])
    nodes = ph._mesh_times(bins, np.array([3, 2, 4]), before[0, 5], before[-1, 5])
    want = np.column_stack([np.interp(nodes, before[:, 5], before[:, c]) for c in range(8)])
    want[:, 5] = nodes
    assert np.array_equal(ph.ActiveTraj, want) and ph.numDefects == 9


def test_table_argument_errors_are_raised_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", no_device)                  # neither the kernels nor the device may be reached
    ode = ShuttleReentry()
    good = synth.make_traj("reentry", "LGL7", 4)
    with pytest.raises(ValueError, match="8 columns"):
        interp.LGLInterpTable(ode, good[:, :-1], "LGL7")
    with pytest.raises(ValueError, match="K\\*nb\\+1"):
        interp.LGLInterpTable(ode, good[:-1], "LGL7")            # 12 rows: not 3 nb + 1
    with pytest.raises(ValueError, match="K\\*nb\\+1"):
        interp.LGLInterpTable(ode, good[:1], "LGL3")             # fewer than one block
    with pytest.raises(ValueError, match="K\\*nb\\+1"):
        interp.LGLInterpTable(ode, synth.make_traj("reentry", "LGL5", 4)[:-1], "LGL5")
    with pytest.raises(ValueError):
        interp.LGLInterpTable(ode, good, "LGL9")
    bad = good.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        interp.LGLInterpTable(ode, bad, "LGL7")


@pytest.mark.parametrize("mode", ["Trapezoidal", "LGL3", "LGL5", "LGL7"])
def test_nddistribute_times_are_the_phases_mesh_times(mode):
    ph = ShuttleReentry().phase(mode)
    bins, per = np.array([0.0, 0.13, 0.2, 0.71, 1.0]), np.array([3, 1, 5, 2])
    for t0, tf in ((0.0, 10.0), (-3.5, 1.25), (7.0, 2.0)):       # (the last one: time running backwards)
        got = interp.distribute_times(mode, bins, per, t0, tf)
        assert np.array_equal(got, ph._mesh_times(bins, per, t0, tf))
        assert got.size == (synth.MODE_CS[mode] - 1) * per.sum() + 1 and got[0] == t0 and got[-1] == tf
