"""The head of the resident pair kernel (csrc/defect_resident.h): the gather that forms the constant rows of both
regions without a load of their own, and the cardinal value phase that runs beside it.  (The looped pair kernel has the same head
once per group and no path of its own here: not among the cases.)  Every block of all five evaluation kinds against the oracle, with
the bounds of tests/test_gpu_parity.py, on the meshes at which a wave of the pair has no segment, one, or shares of one and two."""
import numpy as np
import pytest

from asset_asrl_amd import _lib
from asset_asrl_amd.evaluator import CON, CON_ADJGRAD, JAC, JAC_ADJGRAD, JAC_ADJGRAD_HESS, DefectEvaluator, unpack_kkt_block
from helpers import Workload
from test_gpu_parity import _check_blocks

pytestmark = pytest.mark.gpu

KINDS = (JAC_ADJGRAD_HESS, CON, CON_ADJGRAD, JAC, JAC_ADJGRAD)
WITH_L = (CON_ADJGRAD, JAC_ADJGRAD, JAC_ADJGRAD_HESS)


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _first_alt(cus):
    """(smallest mesh on which Reentry-LGL7 takes the flagship's instantiation -- K_RES_ALT: one group, rows, pair -- on a device of
    ``cus`` compute units, its workgroups): from the planner, as tests/test_launch_plan_cpu.py asks it."""
    def slot(nseg):
        steps, _ = _lib.launch_plan("reentry", _lib.LGL7, False, JAC_ADJGRAD_HESS, False, nseg, cus)
        return [s[0] for s in steps], steps[0][1]
    lo, hi = 1, 10000                     # (the flagship mesh takes it: asserted below)
    assert slot(hi)[0] == ["K_RES_ALT"] and slot(lo)[0] != ["K_RES_ALT"]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if slot(mid)[0] == ["K_RES_ALT"]:
            hi = mid
        else:
            lo = mid
    return hi, slot(hi)[1]


def _all_kinds(oracle, ode, mode, nseg, blocked):
    w = Workload(ode, mode, nseg, blocked, var_offset=3, con_offset=2, extra_vars=4)
    nlp = w.oracle_nlp(oracle, threads=8)
    ev = DefectEvaluator(ode, mode, w.blocked, w.vindex, w.cindex, w.n_primal, w.n_equal)
    for what in KINDS:
        ref = nlp.eval_blocks(what, w.X, w.L)
        got = ev.eval(what, w.X, w.L if what in WITH_L else None)     # (CON and JAC: L = None)
        if what in (JAC, JAC_ADJGRAD):
            H, _ = unpack_kkt_block(got[2][0], w.IR, w.OR)
            assert np.abs(H).max() == 0.0
        _check_blocks(got, ref, w, what)
    ev.close()


@pytest.mark.parametrize("nseg", [1, 2, 3, 5, 17])
def test_reentry_lgl7_blockconstant_small_groups(oracle, nseg):
    """The row-wise part with the early C passes at any size; a phase parameter block (p > 0: P1 reads through the index form);
    groups in which one wave of the pair has no segment, or one."""
    _all_kinds(oracle, "reentry", "LGL7", nseg, True)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_reentry_lgl7_first_meshes_of_the_flagship_form(oracle, which):
    """The smallest meshes of the flagship's own instantiation: shares of one and two segments (t, t + 1, and one short of three
    segments per workgroup)."""
    t, nwg = _first_alt(_cus())
    nseg = (t, t + 1, 3 * nwg - 1)[which]
    steps, _ = _lib.launch_plan("reentry", _lib.LGL7, False, JAC_ADJGRAD_HESS, False, nseg, _cus())
    assert [s[0] for s in steps] == ["K_RES_ALT"] and 2 * steps[0][1] < nseg < 4 * steps[0][1]
    _all_kinds(oracle, "reentry", "LGL7", nseg, False)


@pytest.mark.parametrize("small", [True, False])
def test_reentry_lgl7_renumbered_index_rows_are_not_runs(small):
    """The solver vector renumbered by a random permutation (tests/test_gpu_parity.py: test_renumbered_variables_give_the_same_blocks):
    the gather takes two trips, index then value, P1 reads through the tables -- and the blocks are those of the plain numbering, bit for bit."""
    nseg = 3 if small else _first_alt(_cus())[0]
    w = Workload("reentry", "LGL7", nseg, False, var_offset=3, con_offset=2, extra_vars=4)
    ev = DefectEvaluator("reentry", "LGL7", False, w.vindex, w.cindex, w.n_primal, w.n_equal)
    ref = [a.copy() for a in ev.eval(JAC_ADJGRAD_HESS, w.X, w.L)]
    ref0 = ev.eval(CON, w.X)[0].copy()
    ev.close()
    rng = np.random.default_rng(3)
    pv, pc = rng.permutation(w.n_primal), rng.permutation(w.n_equal)
    X2, L2 = np.empty_like(w.X), np.empty_like(w.L)
    X2[pv], L2[pc] = w.X, w.L
    ev2 = DefectEvaluator("reentry", "LGL7", False, pv[w.vindex].astype(np.int32), pc[w.cindex].astype(np.int32), w.n_primal, w.n_equal)
    got = ev2.eval(JAC_ADJGRAD_HESS, X2, L2)
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ev2.eval(CON, X2)[0], ref0)
    ev2.close()


@pytest.mark.parametrize("ode,mode,blocked,nseg", [("twobody_lt", "LGL5", True, 2), ("twobody_lt", "LGL5", True, 257),
                                                   ("reentry", "Trapezoidal", False, 1), ("reentry", "Trapezoidal", False, 2),
                                                   ("reentry", "Trapezoidal", False, 100)])
def test_constant_rows_of_both_regions_and_the_one_phase_form(oracle, ode, mode, blocked, nseg):
    """Both regions' rows 1 - s_i, s_i, 0, 1 enter every block through the time columns; Trapezoidal: the gather gates the only ODE phase."""
    _all_kinds(oracle, ode, mode, nseg, blocked)
