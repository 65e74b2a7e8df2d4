"""Mesh-error estimation of a phase trajectory on the device.

``mesh_error_integrator`` is the reference's second estimator (``get_meshinfo_integrator``, ODEPhase.h:592-685): every node interval
integrated again with the Prince-Dormand 8(7) pair (csrc/integ_kernels.h), configured by an ``IntegratorOptions``.

``mesh_error_deboor`` is the de Boor estimator of the reference (``ODEPhase<DODE>::get_meshinfo_deboor``,
/root/reference/src/OptimalControl/ODEPhase.h:442-585); ``mesh_info`` adds what ``ODEPhaseBase::getMeshInfo`` does
with it on the host (ODEPhaseBase.h:1355-1399): per-block infinity norms, the cumulative node-density integral and
the equidistributed bin edges for ``n`` new segments."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

_dp = C.POINTER(C.c_double)


def mesh_error_deboor(ode_name: str, mode: str, traj, blocked: bool = False, device: int = 0):
    """Returns (tsnd[nb+1], mesh_errors[XV, nb+1], mesh_dist[XV, nb+1], error[nb+1], dist[nb+1])."""
    T = np.ascontiguousarray(traj, dtype=np.float64)
    xv, uv, pv = _lib.ode_sizes(ode_name)
    if T.ndim != 2 or T.shape[1] != xv + 1 + uv + pv:
        raise ValueError(f"trajectory rows must have {xv + 1 + uv + pv} columns [x,t,u,p]")
    blocked = bool(blocked) and uv > 0      # without controls there is nothing to hold constant (jit.ensure_kernel registers this form)
    cs = 2 if mode == "Trapezoidal" else _lib.MODES[mode]
    nb = (T.shape[0] - 1) // (cs - 1)
    tsnd = np.empty(nb + 1)
    err, dist = np.empty((nb + 1, xv)), np.empty((nb + 1, xv))
    emax, dmax = np.empty(nb + 1), np.empty(nb + 1)
    p = lambda a: a.ctypes.data_as(_dp)
    _lib.check(_lib.lib().asset_hip_mesh_error_deboor(ode_name.encode(), _lib.MODES[mode], int(blocked), p(T), T.shape[0],
                                                      p(tsnd), p(err), p(dist), p(emax), p(dmax), int(device)),
               "asset_hip_mesh_error_deboor")
    return tsnd, err.T.copy(), dist.T.copy(), emax, dmax


class IntegratorOptions:
    """The settings of the re-integrator (the reference's ``phase.integrator``: Integrators/Integrator.h:297-362) with its phase
    defaults (ODEPhase.h:49): DefStepSize 0.01, MinStepSize def / 1e4, MaxStepSize def * 1e4, MaxStepChange 3, Adaptive, AbsTols 1e-12,
    RelTols 0; ``MaxSteps`` (accepted + rejected per node interval) is this project's: the reference has no cap."""

    def __init__(self, xv: int, def_step: float = 0.01):
        self.xv = int(xv)
        self.MaxStepChange, self.Adaptive, self.MaxSteps = 3.0, True, 100000
        self.setStepSizes(def_step, def_step / 10000, def_step * 10000)
        self.setAbsTol(1.0e-12)
        self.setRelTol(0.0)

    def setAbsTol(self, tol: float):
        self.AbsTols = np.full(self.xv, abs(float(tol)))

    def setRelTol(self, tol: float):
        self.RelTols = np.full(self.xv, abs(float(tol)))

    def _tols(self, tols):
        t = np.asarray(tols, dtype=float).ravel()
        if t.size != self.xv:
            raise ValueError("Incorrectly sized tolerance vector.")
        return t.copy()

    def setAbsTols(self, tols):
        self.AbsTols = self._tols(tols)

    def setRelTols(self, tols):
        self.RelTols = self._tols(tols)

    def setStepSizes(self, defstep: float, minstep: float, maxstep: float):
        defstep, minstep, maxstep = float(defstep), float(minstep), float(maxstep)
        if defstep < minstep:
            raise ValueError("Default integrator stepsize must be greater than minimum stepsize.")
        if defstep > maxstep:
            raise ValueError("Default integrator stepsize must be less maximum stepsize.")
        if minstep > maxstep:
            raise ValueError("Minimum integrator stepsize must be greater than minimum stepsize.")
        if defstep < 0 or minstep < 0 or maxstep < 0:
            raise ValueError("Stepsizes must be positive numbers (this doesnt mean you cant integrate backwards).")
        self.DefStepSize, self.MinStepSize, self.MaxStepSize = defstep, minstep, maxstep

    def _c(self):
        """(asset_hip_integ_options, the arrays it points into)"""
        a, r = (np.ascontiguousarray(v, dtype=np.float64) for v in (self.AbsTols, self.RelTols))
        if a.size != self.xv or r.size != self.xv:
            raise ValueError("Incorrectly sized tolerance vector.")
        o = _lib.IntegOptions(self.DefStepSize, self.MinStepSize, self.MaxStepSize, float(self.MaxStepChange), int(bool(self.Adaptive)),
                              int(self.MaxSteps), a.ctypes.data_as(_dp), r.ctypes.data_as(_dp))
        return o, (a, r)


def mesh_error_integrator(ode_name: str, mode: str, traj, blocked: bool = False, options: IntegratorOptions = None, device: int = 0,
                          details: bool = False):
    """Returns (tsnd[nb+1], mesh_errors[XV, nb+1], mesh_dist[XV, nb+1], error[nb+1], dist[nb+1]); with ``details`` also
    (xend[nnodes-1, XV], steps[nnodes-1, 2] accepted / rejected, status[nnodes-1]: 0 ok, 1 step limit, 2 non-finite)."""
    T = np.ascontiguousarray(traj, dtype=np.float64)
    xv, uv, pv = _lib.ode_sizes(ode_name)
    if T.ndim != 2 or T.shape[1] != xv + 1 + uv + pv:
        raise ValueError(f"trajectory rows must have {xv + 1 + uv + pv} columns [x,t,u,p]")
    if options is not None and options.xv != xv:
        raise ValueError("Incorrectly sized tolerance vector.")
    blocked = bool(blocked) and uv > 0
    cs = 2 if mode == "Trapezoidal" else _lib.MODES[mode]
    nb, nint = max((T.shape[0] - 1) // (cs - 1), 0), max(T.shape[0] - 1, 0)
    tsnd = np.empty(nb + 1)
    err, dist = np.empty((nb + 1, xv)), np.empty((nb + 1, xv))
    emax, dmax = np.empty(nb + 1), np.empty(nb + 1)
    xend, steps, status = np.empty((nint, xv)), np.empty((nint, 2), dtype=np.int32), np.empty(nint, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(_dp)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    opt, keep = options._c() if options is not None else (None, None)
    _lib.check(_lib.lib().asset_hip_mesh_error_integrator(ode_name.encode(), _lib.MODES[mode], int(blocked), p(T), T.shape[0],
                                                          C.byref(opt) if opt is not None else None, p(tsnd), p(err), p(dist), p(emax),
                                                          p(dmax), p(xend), ip(steps), ip(status), int(device)),
               "asset_hip_mesh_error_integrator")
    del keep
    out = (tsnd, err.T.copy(), dist.T.copy(), emax, dmax)
    return out + (xend, steps, status) if details else out


def bins_from_density(tsnd, error, dist, n: int):
    """(tsnd, bins, error): cumulative node-density integral and the equidistributed edges of ``n`` new segments
    (ODEPhaseBase.h:1372-1398)."""
    distint = np.zeros_like(dist)
    distint[1:] = np.cumsum(dist[:-1] * np.diff(tsnd))
    distint /= distint[-1]
    bins = np.linspace(0.0, 1.0, n + 1)
    elem = 0
    for i in range(1, n):
        di = i / n
        elem = int(np.searchsorted(distint[elem:], di, side="right")) + elem - 1     # std::upper_bound from `elem`
        t0, t1, d0, d1 = tsnd[elem], tsnd[elem + 1], distint[elem], distint[elem + 1]
        bins[i] = (di - d0) / ((d1 - d0) / (t1 - t0)) + t0
    return tsnd, bins, error


def mesh_info(ode_name: str, mode: str, traj, n: int, blocked: bool = False, device: int = 0):
    """(tsnd, bins, error) -- ODEPhaseBase::getMeshInfo(False, n)."""
    tsnd, _, _, error, dist = mesh_error_deboor(ode_name, mode, traj, blocked, device)
    return bins_from_density(tsnd, error, dist, n)


class MeshIterateInfo:
    """One iterate of the adaptive mesh loop (MeshIterateInfo.h:6-86): the estimate on the current mesh, its summary numbers and the
    cumulative error-density integral the next mesh's edges are read from."""

    def __init__(self, numsegs: int, tol: float, times, error, distribution):
        self.numsegs = self.up_numsegs = int(numsegs)
        self.tol, self.converged, self.global_error = float(tol), False, -1.0
        self.times, self.error, self.distribution = (np.asarray(v, dtype=float).copy() for v in (times, error, distribution))
        hs = np.diff(self.times)
        self.max_error = float(self.error.max())
        self.avg_error = float((self.error[:-1] * hs).sum())
        self.gmean_error = float(np.exp((np.log(self.max_error) + np.log(self.avg_error)) / 2.0))
        self.distintegral = np.zeros_like(self.times)
        self.distintegral[1:] = np.cumsum(self.distribution[:-1] * hs)
        self.distintegral /= self.distintegral[-1]

    def calc_bins(self, nbins: int):
        return bins_from_density(self.times, self.error, self.distribution, int(nbins))[1]
