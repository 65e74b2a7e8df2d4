"""``LGLInterpTable`` -- the transcription's own Hermite interpolant of a trajectory, resident on the device.

The reference's ``LGLInterpTable`` for exact data (/root/reference/src/OptimalControl/LGLInterpTable.h:349-372 ``loadExactData``,
:395-445 ``NDequidist`` / ``NDdistribute`` / ``InterpRange``, :480-669 ``Interpolate`` / ``InterpolateDeriv``): the ODE right-hand
side at every node, then per query time the degree ``2 CS - 1`` polynomial through the values and slopes at the ``CS`` cardinal
nodes of the block that holds the time.  Creation and evaluation are device kernels (csrc/interp_kernels.h behind
``asset_hip_traj_table_*``, include/asset_hip.h); there is no host fallback.  It is the table ``Phase.refineTrajManual`` /
``updateMesh`` re-distribute through with ``setTrajInterpolation("transcription")`` and what ``Phase.returnTrajTable`` returns.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib

_dp = C.POINTER(C.c_double)
_MODE_CS = {"Trapezoidal": 2, "LGL3": 2, "LGL5": 3, "LGL7": 4}


def distribute_times(mode: str, DefBinSpacing, DefsPerBin, t0: float, tf: float) -> np.ndarray:
    """Times of the ``K * sum(DefsPerBin) + 1`` states of a mesh on ``[t0, tf]``: bin ``i`` spans
    ``[DefBinSpacing[i], DefBinSpacing[i+1]]`` (non-dimensional), its ``DefsPerBin[i]`` segments are equal, the states of a segment
    sit at the scheme's cardinal spacing (``NDdistribute``, LGLInterpTable.h:418-433; the rule of ``Phase._mesh_times``)."""
    DBS, DPB = np.asarray(DefBinSpacing, dtype=float).ravel(), np.asarray(DefsPerBin, dtype=int).ravel()
    cs = _MODE_CS[mode]
    tc, K = _lib.lgl_table(cs, "tc"), cs - 1
    edges = np.concatenate([np.linspace(DBS[i], DBS[i + 1], DPB[i] + 1)[(1 if i else 0):] for i in range(DPB.size)])
    edges = t0 + (edges - DBS[0]) / (DBS[-1] - DBS[0]) * (tf - t0)
    nodes = np.empty(K * (edges.size - 1) + 1)
    for j in range(K):
        nodes[j:-1:K] = edges[:-1] + tc[j] * (edges[1:] - edges[:-1])
    nodes[-1] = tf
    return nodes


class LGLInterpTable:
    """``LGLInterpTable(ode, traj, mode="LGL3", blocked=False, device=0)``.

    ``ode``: an :class:`~asset_asrl_amd.ode.ODEBase` (library ODEs are linked in, any other gets device code on first use) or
    the device name of one that is registered.  ``traj``: ``K nb + 1`` node rows ``[x, t, u, p]`` (``K = CS - 1``), times strictly
    monotonic in either direction; block ``e`` is rows ``e K ... e K + CS - 1``.  Any trajectory with two or more rows is a valid
    ``"LGL3"`` table (the reference's default for raw data); ``"Trapezoidal"`` uses the LGL3 table.  ``blocked``: BlockConstant
    control -- controls and ODE parameters of a query are those of its block's first row.

    A time on an interior block boundary belongs to the block that ends there; a time outside ``[T0, TF]`` is extrapolated from
    the first / last block, and such a call warns once (``WarnOutOfBounds``, default on) or raises (``ThrowOutOfBounds``)."""

    def __init__(self, ode, traj, mode: str = "LGL3", blocked: bool = False, device: int = 0):
        if mode not in _MODE_CS:
            raise ValueError("Invalid Transcription Method")
        T = np.ascontiguousarray(traj, dtype=np.float64)
        if isinstance(ode, str):
            name, (xv, uv, pv) = ode, _lib.ode_sizes(ode)
        else:
            name, xv, uv, pv = None, ode.XVars(), ode.UVars(), ode.PVars()
        ncols, K = xv + 1 + uv + pv, _MODE_CS[mode] - 1
        if T.ndim != 2 or T.shape[1] != ncols:
            raise ValueError(f"trajectory rows must have {ncols} columns [x,t,u,p]")
        if T.shape[0] < 2 or (T.shape[0] - 1) % K != 0:
            raise ValueError(f"a {mode} table holds K*nb+1 node rows with K = {K} and nb >= 1 blocks, not {T.shape[0]}")
        if not np.all(np.isfinite(T)):
            raise ValueError("NaN or Inf detected in input trajectory")
        self.mode, self.device = mode, int(device)
        self.BlockedControls = bool(blocked) and uv > 0
        self.XVars, self.UVars, self.PVars, self.XtUPVars = xv, uv, pv, ncols
        self.WarnOutOfBounds, self.ThrowOutOfBounds = True, False
        self._h = None
        if name is None:
            from . import jit
            name = jit.ensure_kernel(ode, mode, self.BlockedControls)
        self.ode_name = name
        h = C.c_void_p()
        _lib.check(_lib.lib().asset_hip_traj_table_create(name.encode(), _lib.MODES[mode], int(self.BlockedControls),
                                                          T.ctypes.data_as(_dp), T.shape[0], self.device, C.byref(h)),
                   "asset_hip_traj_table_create")
        self._h = h
        nb, nc, t0, tf = C.c_int(), C.c_int(), C.c_double(), C.c_double()
        _lib.check(_lib.lib().asset_hip_traj_table_info(h, C.byref(nb), C.byref(nc), C.byref(t0), C.byref(tf)),
                   "asset_hip_traj_table_info")
        self.NumBlocks, self.T0, self.TF = nb.value, t0.value, tf.value

    # ---- life time --------------------------------------------------------------------------------------------
    def close(self):
        if self._h:
            _lib.lib().asset_hip_traj_table_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        """The ``asset_hip_traj_table_t`` (for ``asset_hip_traj_table_interp_device`` with buffers of the caller's own)."""
        if not self._h:
            raise _lib.AssetHipError("the trajectory table is closed")
        return self._h

    # ---- evaluation ---------------------------------------------------------------------------------------------
    def _interp(self, times, deriv: bool):
        t = np.ascontiguousarray(times, dtype=np.float64).ravel()
        if not np.all(np.isfinite(t)):
            raise ValueError("NaN or Inf among the query times")
        out = np.empty((t.size, self.XtUPVars))
        dout = np.empty((t.size, self.XtUPVars)) if deriv else None
        nout = C.c_longlong(0)
        _lib.check(_lib.lib().asset_hip_traj_table_interp(self.handle, t.ctypes.data_as(_dp), t.size, int(deriv),
                                                          out.ctypes.data_as(_dp), dout.ctypes.data_as(_dp) if deriv else None,
                                                          C.byref(nout)), "asset_hip_traj_table_interp")
        self.last_outside = int(nout.value)
        if nout.value:
            msg = (f"{nout.value} of {t.size} query times lie outside the table's range [{self.T0}, {self.TF}]: "
                   "extrapolated from the end blocks")
            if self.ThrowOutOfBounds:
                raise ValueError(msg)
            if self.WarnOutOfBounds:
                warnings.warn(msg, RuntimeWarning, stacklevel=3)
        return out, dout

    def Interpolate(self, t):
        """Scalar ``t`` -> the state vector ``[N]``; array of ``n`` times -> ``[n, N]``."""
        out, _ = self._interp(t, False)
        return out[0] if np.ndim(t) == 0 else out

    __call__ = Interpolate

    def InterpolateDeriv(self, t):
        """Scalar ``t`` -> ``[N, 2]`` (value, time derivative); array of ``n`` times -> the pair ``([n, N], [n, N])``.  The time
        entry's derivative is 1; with BlockConstant control the derivative of controls and parameters is 0 (the derivative of the
        values returned -- the reference's ``InterpolateDeriv`` ignores ``BlockedControls`` and returns the control polynomial)."""
        out, dout = self._interp(t, True)
        return np.column_stack([out[0], dout[0]]) if np.ndim(t) == 0 else (out, dout)

    def NDequidist_times(self, n: int, lo: float, hi: float) -> np.ndarray:
        return distribute_times(self.mode, [0.0, 1.0], [int(n)], self.T0 + lo * (self.TF - self.T0), self.T0 + hi * (self.TF - self.T0))

    def NDequidist(self, n: int, lo: float, hi: float) -> np.ndarray:
        """The ``n K + 1`` cardinal-spaced nodes of ``n`` equal segments between the non-dimensional times ``lo`` and ``hi``
        (0 = T0, 1 = TF; LGLInterpTable.h:395-417)."""
        if int(n) < 1:
            raise ValueError("Number of segments must be positive")
        return self.Interpolate(self.NDequidist_times(n, lo, hi))

    def InterpRange(self, n: int, tl: float, th: float) -> np.ndarray:
        """``NDequidist`` between the dimensional times ``tl`` and ``th`` (LGLInterpTable.h:438-442)."""
        tt = self.TF - self.T0
        return self.NDequidist(n, (tl - self.T0) / tt, (th - self.T0) / tt)

    def InterpWholeRange(self, n: int) -> np.ndarray:
        return self.NDequidist(n, 0.0, 1.0)

    def NDdistribute(self, DefBinSpacing, DefsPerBin) -> np.ndarray:
        """The trajectory on the mesh of ``distribute_times`` over ``[T0, TF]`` (LGLInterpTable.h:418-436)."""
        out = self.Interpolate(distribute_times(self.mode, DefBinSpacing, DefsPerBin, self.T0, self.TF))
        return out
