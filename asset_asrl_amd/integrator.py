"""``ode.integrator(...)``: batched propagation of an ODE on the device (csrc/propagate_kernels.h; include/asset_hip.h:
asset_hip_propagate, asset_hip_propagate_stm).

The reference's ``Integrator`` (Integrators/Integrator.h) in its own method names and return shapes, for the integrator WITHOUT a
controller: rows go in and come out as full ``[x, t, u, p]`` rows, and the controls and parameters of a row are held for the whole
propagation (Integrator.h:204-209).  The method is the Prince-Dormand 8(7) pair ("DOPRI87", also "DP87") with the reference's step
controller; the settings are a :class:`~asset_asrl_amd.mesh.IntegratorOptions` -- the reference's setters and defaults
(Integrator.h:158-172, 297-310) -- plus ``MaxSteps``, this project's cap on accepted + rejected steps of one propagation.

Every call is one batch on the device: a lane per problem (``integrate_parallel``, ``integrate_dense_parallel``) or a lane per
(problem, sensitivity column) (``integrate_stm_parallel``).  A wave of 64 lanes runs as long as its slowest lane, so ORDER SIMILAR
PROBLEMS NEXT TO EACH OTHER: consecutive rows share a wave.

Dense output: ``integrate_dense(x0, tf, n)`` returns the states at ``n`` equally spaced times, each reached by shortening the step
that would pass it -- integrator-accurate, not interpolated.  The reference integrates once and interpolates its step table
(Integrator.h:1917-1946); the end state of a dense call here therefore agrees with ``integrate`` to the tolerance, not bitwise.

State-transition matrix: ``J`` has the reference's layout ``[XV, XV + 1 + UV + PV + 1]``, columns ``[x0 | t0 | u | p | tf]``
(Integrator.h:197).  The ``x0``, ``u`` and ``p`` columns are the exact derivative of the discrete map with the accepted step sequence
held fixed (what the reference chains step by step, Integrator.h:1317-1349); the two time columns are the flow's,
``-S_x f(x0, t0, u, p)`` and ``f(xf, tf, u, p)``.

Out of scope: events; ``integrate_stm2`` (second derivatives); controllers other than held controls (a trajectory's control table);
DOPRI54; ``calc_global_error`` (one serial propagation, not a batch).  ``Phase.AutoScaling`` does not enter: this is an ODE-level
feature and works in the ODE's own units.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .mesh import IntegratorOptions

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
METHODS = ("DOPRI87", "DP87")
STATUS_TEXT = {1: "the step limit MaxSteps was reached", 2: "the step or a state stopped being finite"}


class IntegrationError(_lib.AssetHipError):
    """A propagation ended with a status other than 0 (``details=True`` returns the statuses instead)."""


def parse_integrator_args(args):
    """(method, def_step) of ``ode.integrator(def_step)`` / ``ode.integrator(method, def_step)``."""
    if len(args) == 1 and not isinstance(args[0], str):
        method, def_step = "DOPRI87", args[0]
    elif len(args) == 2 and isinstance(args[0], str):
        method, def_step = args
    else:
        raise TypeError("integrator(def_step) or integrator(method, def_step)")
    if method == "DOPRI54":
        raise NotImplementedError("DOPRI54 is not implemented on the device: use \"DOPRI87\"")
    if method not in METHODS:
        raise ValueError(f"Unknown integration method {method!r}: expected one of {METHODS}")
    return method, float(def_step)


class Integrator(IntegratorOptions):
    """Returned by ``ODEBase.integrator``.  ``device``: HIP device ordinal of every call."""

    def __init__(self, ode, *args, device: int = 0):
        self.method, def_step = parse_integrator_args(args)
        super().__init__(ode.XVars(), def_step)
        self.ode, self.device = ode, int(device)
        self._uv, self._pv = ode.UVars(), ode.PVars()
        self._name = None

    # ---- plumbing
    def _width(self):
        return self.xv + 1 + self._uv + self._pv

    def _device_name(self):
        """A library ODE goes by name; a user ODE is compiled at run time: its LGL3 module holds the propagation kernels."""
        if self._name is None:
            from . import jit
            self._name = jit.ensure_kernel(self.ode, "LGL3", False)
        return self._name

    def _rows(self, x0s, tfs):
        Y = np.ascontiguousarray(np.atleast_2d(np.asarray(x0s, dtype=np.float64)))
        if Y.ndim != 2 or Y.shape[1] != self._width():
            raise ValueError(f"initial rows must have {self._width()} columns [x,t,u,p]")
        T = np.ascontiguousarray(np.asarray(tfs, dtype=np.float64).ravel())
        if T.size != Y.shape[0]:
            raise ValueError(f"{Y.shape[0]} initial rows but {T.size} final times")
        if Y.shape[0] < 1:
            raise ValueError("at least one initial row is needed")
        return Y, T

    def _raise_unless_ok(self, status):
        bad = np.flatnonzero(status != 0)
        if bad.size:
            raise IntegrationError(f"{bad.size} of {status.size} propagations failed; first: problem {int(bad[0])}, status "
                                   f"{int(status[bad[0]])} ({STATUS_TEXT.get(int(status[bad[0]]), '?')})")

    def _propagate(self, Y, T, ns):
        m, n = Y.shape[0], self.xv
        xs, steps, status = np.empty((m, ns, n)), np.empty((m, 2), dtype=np.int32), np.empty(m, dtype=np.int32)
        opt, keep = self._c()
        _lib.check(_lib.lib().asset_hip_propagate(self._device_name().encode(), Y.ctypes.data_as(_dp), m, T.ctypes.data_as(_dp), int(ns),
                                                  C.byref(opt), xs.ctypes.data_as(_dp), steps.ctypes.data_as(_ip), status.ctypes.data_as(_ip),
                                                  self.device), "asset_hip_propagate")
        del keep
        return xs, steps, status

    def _full_rows(self, Y, T, xs):
        """[m, ns, N] rows: the states, their times (the kernel's own formula), the row's controls and parameters."""
        m, ns, n = xs.shape
        out = np.repeat(Y[:, None, :], ns, axis=1)
        out[:, :, :n] = xs
        t0, H = Y[:, n], T - Y[:, n]
        if ns == 1:
            out[:, 0, n] = T
        else:
            j = np.arange(ns, dtype=np.float64)
            out[:, :, n] = t0[:, None] + (j[None, :] * H[:, None]) / float(ns - 1)
            out[:, -1, n] = T
        return out

    # ---- the reference's methods
    def integrate(self, x0, tf, details: bool = False):
        """The end row ``[xf, tf, u, p]``; with ``details`` also (steps[2], status)."""
        r = self.integrate_parallel([x0], [tf], details=details)
        return (r[0][0], r[1][0], int(r[2][0])) if details else r[0]

    def integrate_parallel(self, x0s, tfs, threads=None, details: bool = False):
        """A list of end rows, one per initial row (``threads`` is accepted and ignored: the batch is one launch); with ``details``
        (rows, steps[m, 2], status[m]) and no exception for a failed problem (its states are NaN)."""
        Y, T = self._rows(x0s, tfs)
        xs, steps, status = self._propagate(Y, T, 1)
        if not details:
            self._raise_unless_ok(status)
        rows = list(self._full_rows(Y, T, xs)[:, 0, :])
        return (rows, steps, status) if details else rows

    def integrate_dense(self, x0, tf, n: int, details: bool = False):
        """A list of ``n`` rows at equally spaced times from ``t0`` to ``tf`` (the first is ``x0``'s row)."""
        r = self.integrate_dense_parallel([x0], [tf], n, details=details)
        return (r[0][0], r[1][0], int(r[2][0])) if details else r[0]

    def integrate_dense_parallel(self, x0s, tfs, n: int, threads=None, details: bool = False):
        """Per initial row a list of ``n`` rows; with ``details`` (lists, steps, status)."""
        n = int(n)
        if n < 2:
            raise ValueError("a dense integration returns at least two rows")
        Y, T = self._rows(x0s, tfs)
        xs, steps, status = self._propagate(Y, T, n)
        if not details:
            self._raise_unless_ok(status)
        trajs = [list(tr) for tr in self._full_rows(Y, T, xs)]
        return (trajs, steps, status) if details else trajs

    def integrate_stm(self, x0, tf, details: bool = False):
        """``(xf row, J)``; with ``details`` also (steps[2], status, the end state as the last lane of the lane group holds it)."""
        r = self.integrate_stm_parallel([x0], [tf], details=details)
        return (r[0][0][0], r[0][0][1], r[1][0], int(r[2][0]), r[3][0]) if details else r[0]

    def integrate_stm_parallel(self, x0s, tfs, threads=None, details: bool = False):
        """A list of ``(xf row, J[XV, XV + 1 + UV + PV + 1])``; with ``details`` (that list, steps[m, 2], status[m], xf_last[m, XV])."""
        Y, T = self._rows(x0s, tfs)
        m, n, N = Y.shape[0], self.xv, self._width()
        xf, jac = np.empty((m, 1, n)), np.empty((m, n, N + 1))
        steps, status = np.empty((m, 2), dtype=np.int32), np.empty(m, dtype=np.int32)
        opt, keep = self._c()
        head = (self._device_name().encode(), Y.ctypes.data_as(_dp), m, T.ctypes.data_as(_dp), C.byref(opt), xf.ctypes.data_as(_dp),
                jac.ctypes.data_as(_dp), steps.ctypes.data_as(_ip), status.ctypes.data_as(_ip))
        if details:                                       # (the diagnostic variant: also the last lane's end state)
            last = np.empty((m, n))
            _lib.check(_lib.lib().asset_hip_propagate_stm_lanes(*head, last.ctypes.data_as(_dp), self.device), "asset_hip_propagate_stm_lanes")
        else:
            _lib.check(_lib.lib().asset_hip_propagate_stm(*head, self.device), "asset_hip_propagate_stm")
        del keep
        if not details:
            self._raise_unless_ok(status)
        rows = self._full_rows(Y, T, xf)[:, 0, :]
        res = [(rows[i], jac[i]) for i in range(m)]
        return (res, steps, status, last) if details else res
