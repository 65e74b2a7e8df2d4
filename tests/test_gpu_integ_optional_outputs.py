"""The integrating entry points of the C ABI called directly, at the smallest sizes that exercise the carving of their device arrays
(csrc/capi/arena.h, capi.hip: IntegCall): one problem and a full wave plus one, one sample and three, one event with one stored
occurrence and two with three, the fewest blocks each estimator accepts.  Every case runs twice -- with every optional output
(steps, status; error_max, dist_max, xend) and with all of them NULL -- and asserts that the mandatory outputs are the same bits,
that every output that was given is written through, and that the margin behind every host array is untouched."""
import ctypes as C

import numpy as np
import pytest

import controller_cases as cc
import event_cases
import interp_checker as ick
from asset_asrl_amd import _lib, jit

pytestmark = pytest.mark.gpu

MARGIN = 16
FILL = {np.float64: -7.25, np.int32: -77}
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _ptr(a):
    return a.ctypes.data_as(_dp if a.dtype == np.float64 else _ip)


def _opts():
    return _lib.IntegOptions(0.01, 1e-6, 100.0, 3.0, 1, 100000, None, None)


def _call(entry, head, outs, optional: bool):
    """``entry(*head, outputs.., device 0)``; outs: (name, dtype, count, is optional) in the order of the arguments.  {name: the
    array as written}, None for an optional output that was not given."""
    bufs = {name: np.full(count + MARGIN, FILL[dtype], dtype=dtype) for name, dtype, count, _ in outs}
    given = {name: optional or not opt for name, _, _, opt in outs}
    L = _lib.lib()
    rc = getattr(L, entry)(*head, *[_ptr(bufs[name]) if given[name] else None for name, _, _, _ in outs], 0)
    assert rc == 0, (entry, rc, L.asset_hip_last_error().decode(errors="replace"))
    res = {}
    for name, dtype, count, _ in outs:
        assert np.all(bufs[name][count:] == FILL[dtype]), f"{entry}: the margin behind {name} was written"
        assert count > 0 and not (given[name] and np.any(bufs[name][:count] == FILL[dtype])), f"{entry}: {name} was not written through"
        res[name] = bufs[name][:count] if given[name] else None
    return res


def _both(entry, head, outs):
    full, bare = _call(entry, head, outs, True), _call(entry, head, outs, False)
    for name, dtype, _, opt in outs:
        if opt:
            assert bare[name] is None and full[name] is not None
        else:
            bits = np.uint64 if dtype == np.float64 else np.uint32
            assert np.array_equal(full[name].view(bits), bare[name].view(bits)), f"{entry}: {name} depends on the optional outputs"
    return full


def _problems(m, width, t_col, seed=7, span=0.5):
    """m rows and final times: short arcs of the library's reentry (width 8: rows of a random trajectory) or of vanderpol (width 5)"""
    if width == 8:
        from asset_asrl_amd import synth
        y0 = np.ascontiguousarray(synth.make_traj("reentry", "LGL3", m, seed=seed, T=1.0)[:m])
        span = 0.1
    else:
        y0 = np.ascontiguousarray(np.random.default_rng(seed + m).uniform(0.5, 1.0, (m, width)))
    assert y0.shape == (m, width)
    return y0, np.ascontiguousarray(y0[:, t_col] + span)


F, I = np.float64, np.int32
TAIL = [("steps", I, 2, True), ("status", I, 1, True)]                              # (counts per problem)


def _per_problem(outs, m):
    return [(name, dtype, per * m, opt) for name, dtype, per, opt in outs]


@pytest.fixture(scope="module")
def ctrl_module():
    return jit.ensure_controller_module(cc.make_ode("vanderpol"), *cc.law("vdp_fb"), compile_only=False)     # rows [x0, x1, t, u, p]


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("m", [1, 65])
def test_propagate(m, ns):
    y0, tf = _problems(m, 8, 5)                                                       # reentry: rows [x(5), t, u(2)]
    opt = _opts()
    r = _both("asset_hip_propagate", (b"reentry", _ptr(y0), m, _ptr(tf), ns, C.byref(opt)), _per_problem([("xs", F, ns * 5, False)] + TAIL, m))
    assert np.all(r["status"] == 0) and np.all(np.isfinite(r["xs"]))


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("m", [1, 65])
def test_propagate_ctrl(ctrl_module, m, ns):
    y0, tf = _problems(m, 5, 2)
    opt = _opts()
    r = _both("asset_hip_propagate_ctrl", (ctrl_module.encode(), _ptr(y0), m, _ptr(tf), ns, C.byref(opt)),
              _per_problem([("xs", F, ns * 2, False), ("us", F, ns, False)] + TAIL, m))
    assert np.all(r["status"] == 0) and np.all(np.isfinite(r["xs"])) and np.all(np.isfinite(r["us"]))


STM = [(False, 1, ""), (False, 65, ""), (True, 1, ""), (True, 65, ""), (False, 3, "_lanes"), (True, 3, "_lanes")]


@pytest.mark.parametrize("ctrl,m,lanes", STM, ids=[f"{'ctrl_' if c else ''}stm{l}-{m}" for c, m, l in STM])
def test_propagate_stm(ctrl_module, ctrl, m, lanes):
    n, N, t_col = (2, 5, 2) if ctrl else (5, 8, 5)
    y0, tf = _problems(m, N, t_col)
    opt = _opts()
    outs = [("xf", F, n, False)] + ([("uf", F, 1, False)] if ctrl else []) + [("jac", F, n * (N + 1), False)] + TAIL + \
        ([("xf_last", F, n, False)] if lanes else [])
    name = ctrl_module.encode() if ctrl else b"reentry"
    r = _both(("asset_hip_propagate_ctrl_stm" if ctrl else "asset_hip_propagate_stm") + lanes, (name, _ptr(y0), m, _ptr(tf), C.byref(opt)),
              _per_problem(outs, m))
    assert np.all(r["status"] == 0) and np.all(np.isfinite(r["jac"]))
    if lanes:
        assert np.all(np.isfinite(r["xf_last"]))


@pytest.mark.parametrize("ne,locs", [(1, 1), (2, 3)])
@pytest.mark.parametrize("m", [1, 65])
def test_propagate_events(m, ne, locs):
    names = ("x1", "pos")[:ne]
    module = jit.ensure_event_module(event_cases.make_ode("vanderpol"), [event_cases.event_function("vanderpol", e) for e in names],
                                     compile_only=False)
    y0, tf = _problems(m, 5, 2, span=4.0)
    opt = _opts()
    direction, stop = np.zeros(ne, dtype=I), np.zeros(ne, dtype=I)
    occ = ne * locs
    outs = [("xf", F, 2, False), ("t_end", F, 1, False), ("stopped", I, 1, False), ("ev_count", I, ne, False), ("ev_rows", F, occ * 3, False),
            ("ev_resid", F, occ, False), ("ev_conv", I, occ, False)] + TAIL
    r = _both("asset_hip_propagate_events", (module.encode(), _ptr(y0), m, _ptr(tf), C.byref(opt), ne, _ptr(direction), _ptr(stop), 1.0e-6, 10, locs),
              _per_problem(outs, m))
    assert np.all(r["status"] == 0) and np.all(np.isfinite(r["xf"])) and np.all(np.isfinite(r["t_end"]))


def test_mesh_error_deboor_with_two_blocks():
    nb, n, cs = 2, 5, ick.MODE_CS["LGL5"]
    traj = np.ascontiguousarray(ick.ragged_traj("reentry", "LGL5", nb, seed=3, T=1.0))
    assert traj.shape == (nb * (cs - 1) + 1, 8)
    outs = [("tsnd", F, nb + 1, False), ("errors", F, (nb + 1) * n, False), ("dist", F, (nb + 1) * n, False), ("error_max", F, nb + 1, True),
            ("dist_max", F, nb + 1, True)]
    _both("asset_hip_mesh_error_deboor", (b"reentry", _lib.MODES["LGL5"], 0, _ptr(traj), traj.shape[0]), outs)


def test_mesh_error_integrator_with_one_block():
    nb, n, cs = 1, 5, ick.MODE_CS["LGL5"]
    traj = np.ascontiguousarray(ick.ragged_traj("reentry", "LGL5", nb, seed=3, T=1.0))
    nint = traj.shape[0] - 1
    assert nint == cs - 1
    opt = _opts()
    outs = [("tsnd", F, nb + 1, False), ("errors", F, (nb + 1) * n, False), ("dist", F, (nb + 1) * n, False), ("error_max", F, nb + 1, True),
            ("dist_max", F, nb + 1, True), ("xend", F, nint * n, True), ("steps", I, nint * 2, True), ("status", I, nint, True)]
    r = _both("asset_hip_mesh_error_integrator", (b"reentry", _lib.MODES["LGL5"], 0, _ptr(traj), traj.shape[0], C.byref(opt)), outs)
    assert np.all(r["status"] == 0)
