"""ASSET optimal-control transcriptions on AMD Instinct GPUs (HIP)."""
from .interp import LGLInterpTable  # noqa: F401
