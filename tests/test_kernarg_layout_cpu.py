"""The parameter list of the evaluation kernels (csrc/eval_args.h), held from both sides without a device.

The launcher fills one EvalKernArgs through eval_args_pack and hands the runtime a pointer to each member; every kernel takes
ASSET_EVAL_PARAMS and forms its EvalArgs again with eval_args_rebuild.  A kernel whose parameters lie elsewhere than the launcher
believes reads -- and writes through -- garbage pointers, so:

  * the offsets and sizes the host struct has (printed by a program of its own, plain g++) are compared with the argument metadata of
    EVERY kernel that takes the list, in the static library and in run-time compiled modules: exact equality;
  * the kernel descriptors say how many dwords arrive preloaded in SGPRs: the whole hot list in the resident and adjoint-gradient
    kernels of a default build, none in the variant built without the compiler option;
  * pack -> rebuild gives every field back (the folded `affine` bit, null pointers, negative run constants), also under
    AddressSanitizer and UBSan.
"""
import glob
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asset_asrl_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernarg_layout as KL  # noqa: E402

PROGRAM = r"""
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "eval_args.h"
using namespace asset_hip;

template <class T> static T* fake(uintptr_t v) { return reinterpret_cast<T*>(v); }

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); failures++; } } while (0)

// what a launch does with the pointer array: the runtime copies sizeof(parameter) bytes from ptrs[i] into the argument segment, the
// kernel reads its parameters from there -- here memcpy into locals of the parameters' types, then the kernels' own rebuild
static EvalArgs through_a_launch(const EvalArgs& a, unsigned nwg) {
  EvalKernArgs k;
  void* ptrs[kEvalParams + 1];
  std::memset(&k, 0xAB, sizeof k);
  eval_args_pack(a, nwg, k, ptrs);
  const double *X, *L; int nseg, nwa, v0, vs, c0, cs; double *KKT, *FX; EvalCold cold;
  std::memcpy(&X, ptrs[0], sizeof X), std::memcpy(&L, ptrs[1], sizeof L), std::memcpy(&nseg, ptrs[2], 4), std::memcpy(&nwa, ptrs[3], 4);
  std::memcpy(&v0, ptrs[4], 4), std::memcpy(&vs, ptrs[5], 4), std::memcpy(&c0, ptrs[6], 4), std::memcpy(&cs, ptrs[7], 4);
  std::memcpy(&KKT, ptrs[8], sizeof KKT), std::memcpy(&FX, ptrs[9], sizeof FX), std::memcpy(&cold, ptrs[10], sizeof cold);
  for (int i = 0; i < kEvalParams; i++) CHECK(ptrs[i] >= (void*)&k && ptrs[i] < (void*)(&k + 1));
  return eval_args_rebuild(X, L, nseg, nwa, v0, vs, c0, cs, KKT, FX, cold);
}

static void same(const EvalArgs& a, const EvalArgs& b, unsigned nwg) {
  CHECK(a.nseg == b.nseg); CHECK(a.X == b.X); CHECK(a.L == b.L); CHECK(a.vindex == b.vindex); CHECK(a.cindex == b.cindex);
  CHECK(a.FX == b.FX); CHECK(a.AGX == b.AGX); CHECK(a.KKT == b.KKT); CHECK(a.work == b.work); CHECK(a.kmap == b.kmap);
  CHECK(a.values == b.values); CHECK(a.stage == b.stage); CHECK(a.nvalues == b.nvalues); CHECK(a.lane_consts == b.lane_consts);
  CHECK(a.lane_consts_res == b.lane_consts_res); CHECK(a.affine == b.affine); CHECK(a.aff_v0 == b.aff_v0); CHECK(a.aff_vs == b.aff_vs);
  CHECK(a.aff_c0 == b.aff_c0); CHECK(a.aff_cs == b.aff_cs); CHECK(a.appl_consts == b.appl_consts); CHECK(a.flags == b.flags);
  CHECK(a.units_gp == b.units_gp); CHECK(b.nwg == int(nwg));
}

int main() {
  // ---- layout: one line per parameter, offset and size as the launcher's struct has them
#define ROW(i, f) std::printf("param %d %zu %zu\n", i, offsetof(EvalKernArgs, f), sizeof(EvalKernArgs::f))
  ROW(0, X); ROW(1, L); ROW(2, nseg); ROW(3, nwg_affine); ROW(4, aff_v0); ROW(5, aff_vs); ROW(6, aff_c0); ROW(7, aff_cs);
  ROW(8, KKT); ROW(9, FX); ROW(10, cold);
  std::printf("params %d\nhot_params %d\nhot_dwords %d\npreload_dwords %d\nsize %zu\n", kEvalParams, ASSET_EVAL_HOT_PARAMS,
              ASSET_EVAL_HOT_DWORDS, ASSET_EVAL_PRELOAD_DWORDS, sizeof(EvalKernArgs));
  // ---- round trip: a distinct value in every field
  EvalArgs a;
  a.nseg = 10007, a.X = fake<const double>(0x1000), a.L = fake<const double>(0x2000), a.vindex = fake<const int>(0x3000);
  a.cindex = fake<const int>(0x4000), a.FX = fake<double>(0x5000), a.AGX = fake<double>(0x6000), a.KKT = fake<double>(0x7000);
  a.work = fake<double>(0x8000), a.kmap = fake<const int>(0x9000), a.values = fake<double>(0xA000), a.stage = fake<double>(0xB000);
  a.nvalues = 123457, a.lane_consts = fake<const void>(0xC000), a.lane_consts_res = fake<const void>(0xD000);
  a.affine = 1, a.aff_v0 = 3, a.aff_vs = 24, a.aff_c0 = 2, a.aff_cs = 15, a.appl_consts = fake<const double>(0xE000);
  a.flags = 1, a.units_gp = 7;
  const unsigned grids[] = {1u, 2u, 1024u, 65535u, 0x7fffffffu};
  for (unsigned nwg : grids)
    for (int affine = 0; affine < 2; affine++) {
      EvalArgs b = a;
      b.affine = affine;
      same(b, through_a_launch(b, nwg), nwg);
      b.L = nullptr, b.KKT = nullptr, b.FX = nullptr, b.AGX = nullptr;                    // value-only kinds, kinds without blocks
      same(b, through_a_launch(b, nwg), nwg);
      b.aff_v0 = -3, b.aff_vs = -24, b.aff_c0 = INT_MIN, b.aff_cs = -1, b.nseg = INT_MAX; // the sign of a run constant is not the folded bit
      same(b, through_a_launch(b, nwg), nwg);
      b = EvalArgs();                                                                     // the defaults of a fresh struct
      b.nseg = 1, b.X = a.X, b.L = nullptr, b.vindex = a.vindex, b.cindex = a.cindex, b.FX = a.FX, b.AGX = nullptr, b.KKT = nullptr,
      b.work = nullptr, b.affine = affine;
      same(b, through_a_launch(b, nwg), nwg);
    }
  std::printf(failures ? "FAILED\n" : "roundtrip ok\n");
  return failures ? 1 : 0;
}
"""


def _run_program(tmp_path, name, flags):
    src, exe = tmp_path / "kernargs.cpp", tmp_path / name
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + flags + [str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "roundtrip ok" in out.stdout and "FAILED" not in out.stdout, out.stdout
    rows = [ln.split() for ln in out.stdout.splitlines()]
    params = [(int(r[2]), int(r[3])) for r in rows if r[0] == "param"]
    scal = {r[0]: int(r[1]) for r in rows if len(r) == 2 and r[0] != "roundtrip"}
    assert len(params) == scal["params"]
    return params, scal


@pytest.fixture(scope="module")
def host_layout(tmp_path_factory):
    return _run_program(tmp_path_factory.mktemp("kernargs"), "kernargs", [])


def test_pack_and_rebuild_give_every_field_back(host_layout):
    params, scal = host_layout
    assert scal["hot_params"] == 10 and params[scal["hot_params"]][0] == 4 * scal["hot_dwords"]      # the hot list: dense, then the struct
    assert all(o % s == 0 for o, s in params[:scal["hot_params"]])                                      # no parameter straddles


def test_pack_and_rebuild_under_sanitizers(tmp_path):
    _run_program(tmp_path, "kernargs_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])


def _check_kernels(path, params, size, preload, need):
    ks = KL.kernels(path)
    assert ks, path
    seen = set()
    for name, k in ks.items():
        assert "NS_8EvalArgsE" not in name, f"{name}: takes the host struct by value"     # (a bundle takes BundleArgs, which holds it)
        if KL.EVAL_MARK not in name:
            continue
        ex = KL.explicit(k["args"])
        assert ex[:len(params)] == params, (path, name, ex)
        rest = ex[len(params):]                                                           # a trailing parameter of the kernel's own
        assert rest in ([], [(size, 4)], [(size, 8)]), (path, name, rest)
        family = next((f for f in ("lgl_resident_kernel", "lgl_adjgrad_kernel", "lgl_defect_kernel", "lgl_wide_dense_kernel",
                                   "lgl_rows_kernel", "lgl_ode_units_kernel", "func_kernel") if f in name), None)
        assert family, name
        seen.add(family)
        if family in ("lgl_resident_kernel", "lgl_adjgrad_kernel"):
            assert k["preload"] == preload, (path, name, k["preload"])
    assert need <= seen, (path, need - seen)


def test_every_kernel_of_the_library_has_the_packers_layout(host_layout):
    params, scal = host_layout
    lib = os.path.join(ROOT, "asset_asrl_amd", "libasset_hip.so")
    assert os.path.exists(lib), "build first (__graft_entry__.build())"
    assert scal["preload_dwords"] == scal["hot_dwords"] == 14
    _check_kernels(lib, params, scal["size"], scal["preload_dwords"],
                   {"lgl_resident_kernel", "lgl_adjgrad_kernel", "lgl_defect_kernel", "lgl_wide_dense_kernel", "lgl_rows_kernel",
                    "lgl_ode_units_kernel"})


def test_run_time_compiled_modules_have_the_packers_layout(host_layout):
    params, scal = host_layout
    jit = os.path.join(CSRC, "gen", "jit")
    lgl = sorted(glob.glob(os.path.join(jit, "*", "module_lgl7_0_*.rtc")))
    fn = sorted(glob.glob(os.path.join(jit, "*", "module_function_0_*.rtc")))
    assert lgl and fn, "no run-time compiled modules in the tree's cache: build first (__graft_entry__.build())"
    _check_kernels(lgl[0], params, scal["size"], scal["preload_dwords"], {"lgl_resident_kernel", "lgl_adjgrad_kernel", "lgl_defect_kernel"})
    _check_kernels(fn[0], params, scal["size"], scal["preload_dwords"], {"func_kernel"})


def test_the_variant_without_the_option_preloads_nothing(tmp_path):
    params, scal = _run_program(tmp_path, "kernargs_off", ["-DASSET_KERNARG_PRELOAD=0"])
    assert scal["preload_dwords"] == 0
    lib = os.path.join(ROOT, "exp_build", "variants", "preload0_reentry", "lib.so")
    assert os.path.exists(lib), "build first (__graft_entry__.build() runs tools/build_variants.py)"
    _check_kernels(lib, params, scal["size"], 0, {"lgl_resident_kernel", "lgl_adjgrad_kernel"})
