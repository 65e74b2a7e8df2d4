"""``asset_asrl_amd.vf`` -- the VectorFunctions surface needed to define ODEs (see functions.py): arguments and segments, arithmetic,
elementary functions, norms and products, ``ifelse`` / comparisons / ``sign``, ``F(G)`` composition, tabulated data over one, two and
three axes (``InterpTable1D`` / ``2D`` / ``3D``), and equations solved for one unknown (``ScalarRootFinder(fx[, dfx], iters, tol)``)."""
from .functions import *  # noqa: F401,F403
from .functions import VectorFunction, MatrixFunction, Arguments  # noqa: F401
from .functions import InterpTable1D, InterpTable2D, InterpTable3D  # noqa: F401
from .functions import ScalarRootFinder  # noqa: F401
