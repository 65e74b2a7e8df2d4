"""CPU tests of the per-entry fixtures of the plain per-application functions (tests/golden/func_entries/, tests/func_checker.py):
the fixture is current (the generator reproduces a file bit for bit, the metadata's kappa is func_checker.KAPPA and the measurement
reproduces it); the oracle -- closed forms and both derivative providers -- stays inside the bound on every entry, with the factor 8
the device is given to spare; every fixture reaches the staging class of csrc/func_kernels.h it is there for; the product's own DSL
definitions are held entry by entry on the host, through ``ir.evaluate`` and through the emitted C; and the check sees a wrong small
entry that the block-wise tolerance of the older function tests does not."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import func_checker as fc
from helpers import rel_err

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NAMES = fc.all_names()

# fixture -> (IR, OR, NKKT, staging class): the table of the issue this fixture answers, and of DESIGN.md section 2
TABLE = {
    "lgl_mesh_spacing3": (3, 1, 9, 64), "lgl_mesh_spacing4": (4, 2, 18, 64), "single_mesh_spacing_ac": (3, 1, 9, 64),
    "pathcon": (6, 2, 33, 64), "pairwise": (4, 1, 14, 64),
    "lgl_integral2_powp": (9, 1, 54, 64), "lgl_integral3_powp": (13, 1, 104, 32), "lgl_integral4_quad2": (12, 1, 90, 32),
    "control_spline3_2": (15, 2, 150, 32), "control_spline4_2": (21, 4, 315, 16), "control_spline4_2_o1": (21, 2, 273, 16),
    "control_spline4_3": (28, 6, 574, 8), "lgl_integral4_wide7": (32, 1, 560, 8), "control_spline4_4": (35, 8, 910, 4),
    "control_spline4_5": (42, 10, 1323, 0),
}


@pytest.fixture(scope="module")
def gen():
    sys.path.insert(0, GOLDEN)
    import make_golden_func_entries as g
    return g


def test_generator_reproduces_a_file_bit_for_bit(gen):
    name = "lgl_mesh_spacing3"
    apps = [gen.compute_application(name, k) for k in range(len(gen.FLAGS))]
    with open(gen.path_of(name), "rb") as f:
        assert gen.file_bytes(name, apps, fc.load(name)["meta"]["constants"]) == f.read()


def test_fixture_has_the_applications_it_promises(gen):
    assert NAMES == sorted(gen.FUNCTIONS) == sorted(TABLE)
    for name in NAMES:
        f = fc.load(name)
        m = f["meta"]
        assert f["x"].shape[0] == 6 and m["flags"] == [gen.PLAIN] * 3 + [gen.NARROW, gen.REVERSED, gen.WIDELAM]
        for k in fc.KINDS:
            assert f[k].dtype == np.float64 and f[k + "E"].dtype == np.float32 and f[k].shape == f[k + "E"].shape
            assert np.all(np.isfinite(f[k])) and np.all(np.isfinite(f[k + "E"])) and np.all(f[k + "E"] >= 0)
        assert f["hx"].shape[1] == f["IR"] * (f["IR"] + 1) // 2 and ("ac" in f) == (m["kind"] == "single_mesh_spacing")
        lam = f["lam"][5]
        assert np.abs(lam).max() == 1e3 and np.sum(lam == 0) == (min(2, f["OR"] - 2) if f["OR"] > 2 else 0)
        assert f["OR"] == 1 or np.abs(lam[lam != 0]).min() == 1e-6
        if m["kind"] == "user":
            continue
        a = m["args"]                                      # the segment widths: narrow and reversed where the flags say so
        tix = {"lgl_mesh_spacing": lambda: (0, f["IR"] - 1), "single_mesh_spacing": lambda: (0, 2),
               "lgl_integral": lambda: (a["xv"], (a["cs"] - 1) * (a["xv"] + 1) + a["xv"]),
               "control_spline": lambda: (0, (a["cs"] - 1) * (a["usize"] + 1))}[m["kind"]]()
        for x, fl in zip(f["x"], m["flags"]):
            h = x[tix[1]] - x[tix[0]]
            assert (h < 0) == bool(fl & gen.REVERSED) and (abs(h) < 1e-3) == bool(fl & gen.NARROW)
    f = fc.load("control_spline4_3")                       # the narrow application: powers of 1 / h from the first to the fourth in one block
    big = np.abs(np.concatenate([f["jx"][3].ravel(), f["hx"][3]]))
    assert big.max() > 1e12 * big[big > 0].min()


def test_every_fixture_reaches_its_staging_class(gen):
    """The Python statement of FuncStage<F>::APW (func_checker.stage_class) over the fixtures: if ASSET_FUNC_LDS_BUDGET is retuned, this
    says which class lost its fixture."""
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "asset_asrl_amd", "csrc", "func_kernels.h")).read()
    assert "#define ASSET_FUNC_LDS_BUDGET (40 * 1024 - 64)" in src and fc.LDS_BUDGET == 40 * 1024 - 64 == gen.LDS_BUDGET
    for name, (ir, orr, nkkt, cls) in TABLE.items():
        f = fc.load(name)
        assert (f["IR"], f["OR"], f["NKKT"]) == (ir, orr, nkkt) and f["meta"]["stage_class"] == cls
        assert fc.stage_class(ir, orr) == cls == gen.stage_class(ir, orr), name
    assert {c for _, _, _, c in TABLE.values()} == {64, 32, 16, 8, 4, 0}
    assert (64 * (104 | 1) * 8 > fc.LDS_BUDGET) and (4 * (1323 | 1) * 8 > fc.LDS_BUDGET)


def test_kappa_is_eight_times_the_measured_oracle_ratio_rounded_up_to_a_power_of_two():
    c = fc.load(NAMES[0])["meta"]["constants"]
    assert c["factor"] == 8.0 and c["inexact"] == 0
    for k in fc.KINDS:
        w = max(c["worst"][k].values())
        assert c["kappa"][k] == fc.pow2_ceil(8.0 * w) == fc.KAPPA[k], (k, w)
    for name in NAMES:                                     # the same record in every file
        assert fc.load(name)["meta"]["constants"] == c


def test_measurement_reproduces_the_recorded_constants(oracle):
    got, c = fc.measure_constants(), fc.load(NAMES[0])["meta"]["constants"]
    assert got["kappa"] == c["kappa"] == fc.KAPPA and got["inexact"] == 0
    for k in fc.KINDS:                                     # (the ratios themselves move with the host's libm; kappa has room: 8 x 0.498)
        for p, w in c["worst"][k].items():
            assert abs(got["worst"][k][p] - w) <= 0.02, (k, p, got["worst"][k][p], w)


@pytest.mark.parametrize("name,provider", [(n, p) for n in NAMES for p, _ in fc.providers(fc.load(n))],
                         ids=[f"{n}-{pn}" for n in NAMES for _, pn in fc.providers(fc.load(n))])
def test_oracle_stays_inside_an_eighth_of_the_bound(oracle, name, provider):
    f = fc.load(name)
    got = fc.oracle_blocks(oracle, f, provider)
    ids = np.arange(f["x"].shape[0])
    for k in fc.KINDS:
        r = fc.check(got[k], f, ids, k)
        assert r["over"] == 0 and 8.0 * r["worst"] <= 1.0, (k, r)
        zero = f[k + "E"] == 0
        assert np.array_equal(got[k].reshape(f[k].shape)[zero], f[k][zero])


def _assert_host(name, route, got):
    f = fc.load(name)
    ids = np.arange(f["x"].shape[0])
    res = {k: fc.check(got[k], f, ids, k) for k in fc.KINDS}
    print(f"[func entries] {name} {route}: worst |got - ref| / bound  " + "  ".join(f"{k} {res[k]['worst']:.3g}" for k in fc.KINDS))
    assert not [(k, r) for k, r in res.items() if r["over"]], (name, route, res)


def _derivatives(name):
    from asset_asrl_amd.vf import codegen
    func, _ = fc.product_function(fc.load(name))
    d = codegen.differentiate_function(name, func)
    assert (d.nin, d.xv) == (fc.load(name)["IR"], fc.load(name)["OR"])
    return d


@pytest.mark.parametrize("name", NAMES)
def test_symbolic_derivatives_of_the_product_definitions_entry_by_entry(name):
    """``ir.evaluate`` over ``codegen.differentiate_function`` of pathfuncs.LGLMeshSpacing ... LGLIntegral(I7, 4, 7): the symbolic
    derivatives of the phase functions at 50 digits, without a GPU."""
    from asset_asrl_amd.vf.ir import evaluate
    f, d = fc.load(name), _derivatives(name)
    N, n = d.nin, d.xv
    roots = d.f + [e for r in d.J for e in r] + d.g + [d.H[i][j] for i in range(N) for j in range(i + 1)]
    rows = np.array([evaluate(roots, f["x"][s], f["lam"][s], f["ac"][s] if "ac" in f else ()) for s in range(f["x"].shape[0])])
    fx, jx, gx, hx = np.split(rows, np.cumsum([n, n * N, N]), axis=1)
    _assert_host(name, "ir.evaluate", dict(fx=fx, jx=jx, gx=gx, hx=hx))


@pytest.mark.parametrize("name", NAMES)
def test_emitted_c_of_the_product_definitions_entry_by_entry(tmp_path, name):
    """``codegen.emit_c`` compiled with gcc -O1, as tests/test_vf_ops_cpu.py compiles it.  A constant of the application (vf.ApplConst)
    is printed as ``c0``: here a global the test sets before each call."""
    from asset_asrl_amd.vf import codegen
    f, d = fc.load(name), _derivatives(name)
    N, n = d.nin, d.xv
    text = codegen.emit_c(d, "fe")
    if "ac" in f:
        text = "double c0;\n" + text
    src, so = tmp_path / "c.c", tmp_path / "c.so"
    src.write_text(text)
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", str(src), "-o", str(so), "-lm"])
    L = C.CDLL(str(so))
    il = np.tril_indices(N)
    out = dict(fx=[], jx=[], gx=[], hx=[])
    for s in range(f["x"].shape[0]):
        if "ac" in f:
            C.c_double.in_dll(L, "c0").value = float(f["ac"][s, 0])
        y, lam = np.ascontiguousarray(f["x"][s]), np.ascontiguousarray(f["lam"][s])
        fx, J, g, H = np.zeros(n), np.zeros((n, N)), np.zeros(N), np.full((N, N), np.nan)
        L.fe_fjgh(*[C.c_void_p(a.ctypes.data) for a in (y, lam, fx, J, g, H)])
        assert np.array_equal(H, H.T)
        for k, v in zip(("fx", "jx", "gx", "hx"), (fx, J, g, H[il])):
            out[k].append(v)
    _assert_host(name, "emit_c", {k: np.stack(v) for k, v in out.items()})


def test_check_sees_a_small_wrong_entry_that_the_block_wise_tolerance_does_not():
    """Why this fixture exists: an entry of a control-spline Hessian six orders below its block's largest one, wrong in its fourth
    digit, passes ``helpers.rel_err < 1e-8`` (tests/test_gpu_function.py, tests/test_gpu_phase_functions.py) and fails the per-entry
    check."""
    f = fc.load("control_spline4_3")
    ids = np.arange(f["x"].shape[0])
    assert fc.check(f["hx"], f, ids, "hx") == dict(worst=0.0, where=(0, 0), over=0, n=f["hx"].size)
    h = f["hx"].copy()
    small = np.argwhere((np.abs(h) < 1e-6 * np.abs(h).max(axis=1, keepdims=True)) & (h != 0))
    assert len(small) > 0
    at = tuple(small[0])
    h[at] *= 1.0 + 1e-3
    assert rel_err(h[at[0]], f["hx"][at[0]]) < 1e-8 and rel_err(h, f["hx"]) < 1e-8
    r = fc.check(h, f, ids, "hx")
    assert r["over"] == 1 and r["where"] == at and r["worst"] > 1e9
    z = np.argwhere(f["hxE"] == 0)                         # a structural zero must be 0.0
    h = f["hx"].copy()
    h[tuple(z[0])] = 1e-300
    assert fc.check(h, f, ids, "hx")["over"] == 1
