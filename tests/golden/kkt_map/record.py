"""Writes kkt_maps.npz beside this file: the outputs of asset_hip_kkt_map_query for the cases of tests/test_kkt_map_cpu.py, with their
inputs.  Run from the repository root, against a build whose build_kkt_map is still the text of asset_hip_defect_set_kkt_map as it
stood before the split (see the docstring of the test); running it against a later build records that build's own answers.

  python tests/golden/kkt_map/record.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from asset_asrl_amd import _lib  # noqa: E402
from oracle import bindings  # noqa: E402
from test_kkt_map_cpu import CASES, case_inputs, kinds_of  # noqa: E402

bindings.build()
out = {"cases": np.array(sorted(CASES))}
for name in sorted(CASES):
    ir, orr, plain, accumulate, locs, nvalues = case_inputs(bindings, name)
    words, ptr, loc, lo, hi = _lib.kkt_map(ir, orr, plain, locs, nvalues, accumulate)
    # (the two long arrays as first differences: neighbouring entries differ by small, repeating steps, which compresses 7x better)
    out.update({name + "/slot_locations.diff": np.diff(locs.ravel().astype(np.int64), prepend=0), name + "/nseg": np.int64(locs.shape[0]),
                name + "/nvalues": np.int64(nvalues), name + "/map_words.diff": np.diff(words.astype(np.int64), prepend=0),
                name + "/multi_ptr": ptr, name + "/multi_loc": loc, name + "/range": np.array([lo, hi], dtype=np.int64)})
    print(name, f"IR={ir} OR={orr} nseg={locs.shape[0]} nvalues={nvalues} words={words.size} staged locations={loc.size}",
          kinds_of(words, nvalues))
np.savez_compressed(os.path.join(HERE, "kkt_maps.npz"), **out)
print(os.path.getsize(os.path.join(HERE, "kkt_maps.npz")), "bytes")
