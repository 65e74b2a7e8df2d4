"""Every kernel family launched through the one argument packer (csrc/eval_args.h, registry.h: launch_eval), against the oracle with
the tolerances of tests/test_gpu_parity.py, at the smallest shapes at which argument passing can differ: index tables that are runs
(the addresses come from preloaded arguments) and tables that are not (they come from the struct part), kinds that pass a null L
or set `flags`, a kernel with a trailing parameter of its own, a run-time compiled module, a plain function, a sharded handle, and a
launch whose workgroup count -- an argument since the kernels stopped reading gridDim -- is far from the mesh size."""
import os
import subprocess
import sys

import numpy as np
import pytest

from asset_asrl_amd import jit
from asset_asrl_amd.evaluator import (CON, CON_ADJGRAD, JAC, JAC_ADJGRAD, JAC_ADJGRAD_HESS, KEEP_HESSIAN_SLOTS, DefectEvaluator,
                                      ShardedDefectEvaluator)
from helpers import Workload, make_shape, rel_err
from test_gpu_parity import _check_blocks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (JAC_ADJGRAD_HESS, CON, CON_ADJGRAD, JAC, JAC_ADJGRAD)
WITH_L = (CON_ADJGRAD, JAC_ADJGRAD, JAC_ADJGRAD_HESS)


def _all_kinds(ev, nlp, w):
    for what in KINDS:
        got = ev.eval(what, w.X, w.L if what in WITH_L else None)      # CON and JAC pass a null L
        _check_blocks(got, nlp.eval_blocks(what, w.X, w.L), w, what)


@pytest.mark.parametrize("ode,mode,nseg,blocked", [
    ("reentry", "LGL7", 1, False), ("reentry", "LGL7", 2, False), ("reentry", "LGL7", 11, False), ("reentry", "LGL7", 21, False),
    ("twobody_lt", "LGL5", 3, True), ("twobody_lt", "LGL5", 11, True),     # BlockConstant: tables that are not runs
    ("reentry", "Trapezoidal", 5, False),
    ("synthetic32", "LGL3", 2, False)])                                    # a wide shape: unit kernels (trailing parameter), four-wave dense part
def test_library_shapes_all_kinds(oracle, ode, mode, nseg, blocked):
    w = Workload(ode, mode, nseg, blocked)
    ev = DefectEvaluator(ode, mode, w.blocked, w.vindex, w.cindex, w.n_primal, w.n_equal)
    nlp = w.oracle_nlp(oracle, threads=2)
    _all_kinds(ev, nlp, w)
    if ode == "reentry" and mode == "LGL7":                                # `flags`: the Jacobian slots are the plain kind's, bit for bit
        plain = [None if a is None else a.copy() for a in ev.eval(JAC_ADJGRAD, w.X, w.L)]
        kept = ev.eval(JAC_ADJGRAD | KEEP_HESSIAN_SLOTS, w.X, w.L)
        hmask = np.zeros(w.NKKT, dtype=bool)
        k = 0
        for i in range(w.IR):
            hmask[k:k + w.IR - i] = True
            k += (w.IR - i) + w.OR
        assert np.array_equal(kept[2][:, ~hmask], plain[2][:, ~hmask]) and np.array_equal(kept[0], plain[0]) and np.array_equal(kept[1], plain[1])
    ev.close()


def test_run_time_compiled_ode(oracle):
    n, m, p, mode = 3, 0, 1, "LGL5"                                        # (tests/test_gpu_shapes.py: CASES)
    name = jit.ensure_kernel(make_shape(n, m, p), mode, False)
    w = Workload(f"shape_{n}_{m}_{p}", mode, 4, False, sizes=(n, m, p), var_offset=2, con_offset=1, extra_vars=3)
    nlp = oracle.Nlp(oracle.get_ode(f"shape_{n}_{m}_{p}", 0), oracle.MODES[mode], w.blocked, w.vindex, w.cindex, w.n_primal, w.n_equal, 2)
    ev = DefectEvaluator(name, mode, w.blocked, w.vindex, w.cindex, w.n_primal, w.n_equal)
    _all_kinds(ev, nlp, w)
    ev.close()


def test_plain_function(oracle):
    from asset_asrl_amd.pathfuncs import FunctionEvaluator
    from test_gpu_function import _pathcon, _tables
    napp, ir, orr = 5, 6, 2
    n_primal, n_equal = 3 * napp + 20, 2 * napp + 5
    vindex, cindex, X, L = _tables(napp, ir, orr, n_primal, n_equal, 11)
    ev = FunctionEvaluator(_pathcon(), "pathcon", vindex, cindex, n_primal, n_equal)
    nlp = oracle.Nlp(oracle.get_ode("pathcon", 0), oracle.MODES["Function"], False, vindex, cindex, n_primal, n_equal, 2)
    for what in KINDS:
        rfx, ragx, rkkt = nlp.eval_blocks(what, X, L)
        fx, agx, kkt = ev.eval(what, X, L if what in WITH_L else None)
        assert np.abs(fx - rfx).max() < 1e-10
        if agx is not None:
            assert rel_err(agx, ragx) < 1e-8
        if kkt is not None:
            assert rel_err(kkt, rkkt) < 1e-8
    ev.close()


def test_sharded_handle_is_bitwise_the_single_handle():
    w = Workload("reentry", "LGL7", 7, False)
    one = DefectEvaluator("reentry", "LGL7", False, w.vindex, w.cindex, w.n_primal, w.n_equal)
    sh = ShardedDefectEvaluator("reentry", "LGL7", False, w.vindex, w.cindex, w.n_primal, w.n_equal, [0, 0])
    for what in KINDS:
        L = w.L if what in WITH_L else None
        for x, y in zip(one.eval(what, w.X, L), sh.eval(what, w.X, L)):
            assert (x is None) == (y is None)
            if x is not None:
                np.testing.assert_array_equal(x, y)
    sh.close()
    one.close()


_SMALL_GRID = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
from helpers import Workload
from asset_asrl_amd.evaluator import JAC_ADJGRAD_HESS, DefectEvaluator
from oracle import bindings as ob
from test_gpu_parity import _check_blocks
ob.build()
for nseg in (41, 51):
    w = Workload("reentry", "LGL7", nseg, False)
    ev = DefectEvaluator("reentry", "LGL7", False, w.vindex, w.cindex, w.n_primal, w.n_equal)
    _check_blocks(ev.eval(JAC_ADJGRAD_HESS, w.X, w.L), w.oracle_nlp(ob, threads=2).eval_blocks(ob.JAC_ADJGRAD_HESS, w.X, w.L), w, JAC_ADJGRAD_HESS)
    ev.close()
print("small grid ok")
"""


def test_share_arithmetic_with_a_small_grid(oracle):
    """ASSET_HIP_RESIDENT_GRID=4 (read once per process, so a child): four waves for 2 GR waves + 1 = 41 segments (GR = 5 for
    Reentry-LGL7) and for 51 -- the looped pair kernel walks two and three groups per wave, every share formed from the explicit count."""
    env = dict(os.environ, ASSET_HIP_TUNING="1", ASSET_HIP_RESIDENT_GRID="4")
    r = subprocess.run([sys.executable, "-c", _SMALL_GRID, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "small grid ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "ASSET_HIP_RESIDENT_GRID=4 is in effect" in r.stderr, r.stderr[-2000:]      # (the library says which knobs it honours)
