"""clock64() deltas of a -DASSET_TIMING build of the pair kernel, Reentry-LGL7 x 10 000, workgroup 7: wave 0 (left in FX) and wave 1 (AGX),
four launches (the first is cold: use 2-4).

  python tools/build_one.py tu_reentry_lgl4_0 build_dbg/libT.so -DASSET_TIMING
  ASSET_HIP_LIB=build_dbg/libT.so python tools/attic/dbg_time_pair.py
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from helpers import Workload
from asset_asrl_amd.evaluator import DefectEvaluator
nseg = 10000
w = Workload("reentry", "LGL7", nseg, False)
ev = DefectEvaluator("reentry", "LGL7", False, w.vindex, w.cindex, w.n_primal, w.n_equal)
nshare = 2048; per = nseg // nshare; rem = nseg % nshare      # (1 024 workgroups of two waves; more extras than workgroups: the plain split)
def first(sh): return sh * per + min(sh, rem)
for rep in range(4):
    fx, agx, kkt = ev.eval(4, w.X, w.L)
    for name, arr, ld, sh in (("wave0/FX", fx, ev.OR, 14), ("wave1/AGX", agx, ev.IR, 15)):
        d = arr.ravel()[first(sh) * ld: first(sh) * ld + 23]
        out = []
        for x in d:
            if x == round(x) and 1 <= abs(x) < 1e7: out.append(int(x))
            else: break
        print(f"rep {rep} {name} segment {first(sh)} deltas {out}", flush=True)
ev.close()
