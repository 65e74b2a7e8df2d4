"""Which kernels an evaluation launches, by mesh size: one markdown table per compiled (ODE, transcription, control mode), from
asset_hip_launch_plan_query (include/asset_hip.h) -- no device.  DESIGN.md section 4.1 "Launch forms" is this script's output.

    python tools/dispatch_table.py [--cus 256] [--max 4000000] [ode ...]

A form is the sequence of (kernel slot, block size) of a plan; grids, LDS sizes and group sizes vary inside an interval
(`python -c "from asset_asrl_amd import _lib; print(_lib.launch_plan('reentry', 4, False, 4, False, 10000))"` shows one plan in full).
Boundaries are found on every mesh size up to 4 096, then by bisection between samples 64 apart (geometric beyond 200 000)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asset_asrl_amd import _lib  # noqa: E402

REQUESTS = [("value", _lib.CON, False), ("value + adjoint gradient", _lib.CON_ADJGRAD, False),
            ("Jacobian, blocks", _lib.JAC_ADJGRAD, False), ("Jacobian, assembled", _lib.JAC_ADJGRAD, True),
            ("Hessian, blocks", _lib.JAC_ADJGRAD_HESS, False), ("Hessian, assembled", _lib.JAC_ADJGRAD_HESS, True)]


def intervals(form, nmax):
    """[(first, last, form)] of form(nseg) over 1..nmax"""
    pts = list(range(1, min(4096, nmax) + 1))
    while pts[-1] < nmax:
        pts.append(min(nmax, pts[-1] + 64 if pts[-1] < 200000 else pts[-1] * 5 // 4))
    vals = {n: form(n) for n in pts}

    def split(a, b):            # form(a) != form(b): every change in (a, b]
        if b == a + 1:
            return [b]
        mid = (a + b) // 2
        vals[mid] = form(mid)
        return (split(a, mid) if vals[a] != vals[mid] else []) + (split(mid, b) if vals[mid] != vals[b] else [])

    starts = [1]
    for a, b in zip(pts, pts[1:]):
        if vals[a] != vals[b]:
            starts += split(a, b)
    return [(s, (starts[i + 1] - 1 if i + 1 < len(starts) else nmax), vals[s]) for i, s in enumerate(starts)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--max", type=int, default=4000000)
    ap.add_argument("odes", nargs="*")
    args = ap.parse_args(argv)
    num = lambda n: f"{n:,}".replace(",", " ")
    one_form = {}               # requests that take one form at every size for every shape: said once, at the end
    for ode in args.odes or _lib.ode_names():
        for mode, mid in _lib.MODES.items():
            for blocked in (False, True):
                if mode == "Function" or not _lib.has_kernel(ode, mid, blocked):
                    continue
                print(f"\n`{ode}` {mode}{' BlockConstant' if blocked else ''} ({args.cus} CUs)\n")
                print("| evaluation | segments: kernels (× threads per workgroup) |\n|---|---|")
                for label, what, assembled in REQUESTS:
                    def form(n):
                        return tuple((s[0], s[3]) for s in _lib.launch_plan(ode, mid, blocked, what, assembled, n, args.cus)[0])
                    iv = intervals(form, args.max)
                    text = lambda f: " + ".join(f"`{k}`×{blk}" for k, blk in f)
                    if what < _lib.JAC and len(iv) == 1:
                        one_form.setdefault(label, set()).add(text(iv[0][2]))
                        continue
                    print(f"| {label} | " + "; ".join(f"{num(a)} – {num(b)}: {text(f)}" for a, b, f in iv) + " |")
    for label, forms in one_form.items():
        print(f"\nEvery shape above, {label}, 1 – {num(args.max)} segments: " + " / ".join(sorted(forms)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
