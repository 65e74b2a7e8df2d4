"""The kinds of a compiled module are ABI (csrc/kernel_meta.h: MF_KIND): ``_lib.KIND_*`` name the integers the library writes into
meta[0] of a cached module of each kind, and every kernel slot belongs to the kinds recorded here -- the bit masks of
asset_hip_kernel_slot_kinds (bit k - 1: modules of kind k have the kernel), as a literal table."""
import ctypes as C
import glob
import os

import pytest

from asset_asrl_amd import _lib, jit

# (kind, the file tag of its cached modules: asset_asrl_amd/jit.py)
KINDS = [(_lib.KIND_LGL, "lgl3_0"), (_lib.KIND_FUNCTION, "function_0"), (_lib.KIND_BUNDLE, "bundle_0"), (_lib.KIND_EVENTS, "events_0"),
         (_lib.KIND_CTRL, "ctrl_0"), (_lib.KIND_EVENTS_STM, "eventstm_0")]

SLOT_KINDS = [
    ("K_LGL1_S1", 1), ("K_LGL2_S1", 1), ("K_LGL1_S2", 1), ("K_LGL1_S2_ASM", 1), ("K_LGL2_S2", 1), ("K_LGL2_S2_ASM", 1), ("K_LGL1_S3", 1),
    ("K_LGL1_S3_ASM", 1), ("K_LGL2_S3", 1), ("K_LGL2_S3_ASM", 1), ("K_LGL2_S4", 1), ("K_LANE_SETUP1", 1), ("K_LANE_SETUP2", 1), ("K_WIDE1", 1),
    ("K_WIDE1_ASM", 1), ("K_WIDE2", 1), ("K_WIDE2_ASM", 1), ("K_WIDE_SETUP", 1), ("K_ROWS1", 1), ("K_ROWS2", 1), ("K_ADJGRAD", 1), ("K_VALUE", 1),
    ("K_RES1", 1), ("K_RES1_ASM", 1), ("K_RES2", 1), ("K_RES2_ASM", 1), ("K_RESL1", 1), ("K_RESL1_ASM", 1), ("K_RESL2", 1), ("K_RESL2_ASM", 1),
    ("K_RESLP", 1), ("K_RES_ALT", 1), ("K_RESD", 1), ("K_RESD_ASM", 1), ("K_RES_SETUP", 1), ("K_UNITS0", 1), ("K_UNITS1", 1), ("K_UNITSJ", 1),
    ("K_UNITS4", 1), ("K_MESH_YVEC", 1), ("K_MESH_ERROR", 1), ("K_INTERP_XDOT", 1), ("K_INTERP_EVAL", 1), ("K_INTEG_STEP", 1),
    ("K_INTEG_ERROR", 1), ("K_FUNC0", 2), ("K_FUNC1", 2), ("K_FUNC1_ASM", 2), ("K_FUNC2", 2), ("K_FUNC2_ASM", 2), ("K_BUNDLE0", 4),
    ("K_BUNDLE1", 4), ("K_BUNDLE2", 4), ("K_PROP_BATCH", 1), ("K_PROP_STM", 1), ("K_PROP_JAC", 1), ("K_PROP_EVENT", 8), ("K_PROP_CTRL_BATCH", 16),
    ("K_PROP_CTRL_STM", 16), ("K_PROP_CTRL_JAC", 16), ("K_PROP_EVENT_STM", 32), ("K_PROP_EVENT_JAC", 32)]


def test_the_named_kinds_are_the_integers_1_to_6():
    assert [k for k, _ in KINDS] == [1, 2, 3, 4, 5, 6]


@pytest.mark.parametrize("kind,tag", KINDS)
def test_a_cached_module_of_each_kind_carries_the_named_integer(kind, tag):
    files = sorted(glob.glob(os.path.join(jit.JIT_DIR, "*", f"module_{tag}_*.rtc")))
    assert files, f"the build caches no module_{tag}_* file"
    meta = (C.c_longlong * 64)()
    assert _lib.lib().asset_hip_rtc_module_meta(files[0].encode(), meta, 64) == 42 and meta[0] == kind


def test_every_kernel_slot_belongs_to_the_kinds_it_belonged_to():
    L = _lib.lib()
    got, s = [], 0
    while L.asset_hip_kernel_slot_name(s) is not None:
        got.append((L.asset_hip_kernel_slot_name(s).decode(), L.asset_hip_kernel_slot_kinds(s)))
        s += 1
    assert got == SLOT_KINDS
    assert L.asset_hip_kernel_slot_kinds(-1) == 0 and L.asset_hip_kernel_slot_kinds(len(got)) == 0
