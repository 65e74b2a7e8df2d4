"""Per-entry check of defect blocks against tests/golden/defect_entries/<shape>.npz (made by
tests/golden/make_golden_defect_entries.py): the 50-digit value of EVERY entry of fx, jx, gx = J^T lam and hx = sum_k lam_k grad^2 d_k
of a few segments of every shape, and for every entry a running error bound E in units of u = 2^-53.  Pure numpy; nothing under test
is touched here.

    bound(E, kind) = kappa_kind * u * E          an entry with E = 0 has no rounded term: it must be EXACTLY the stored value
                                                 (a structural zero must be 0.0)

The four kappa are measured, not chosen (``measure_constants``): the oracle's two derivative providers -- AD2 and the generated
analytic derivatives, the closer relative of the device code -- are run over the whole fixture on the CPU, the worst
|oracle - ref| / (u E) per quantity is multiplied by 8 and rounded up to a power of two.  The factor 8 is the one the mesh fixture
uses, for the same reason: the device functor is generated code with its own operation order and FMA contraction, and the device's
Hessian algorithm (M_i products and the rank-2 time update) is not the AD recursion E models.  The device's own results never enter.
The measured ratios and the constants are in every fixture's metadata (``constants``) and in DESIGN.md section 2;
tests/test_defect_entries_cpu.py holds KAPPA below to them.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "defect_entries")
U = 2.0 ** -53
KINDS = ("fx", "jx", "gx", "hx")          # value, J, J^T lam, H

# 8 x (worst oracle ratio), rounded up to a power of two -- see measure_constants() and the fixtures' metadata
KAPPA = {"fx": 8.0, "jx": 8.0, "gx": 8.0, "hx": 4.0}


def shape_name(ode: str, mode: str, blocked: bool) -> str:
    return f"{ode}_{mode}{'_blocked' if blocked else ''}"


def all_shapes():
    """[(ode, mode, blocked)] of every fixture file, from the files' own metadata"""
    out = []
    for fn in sorted(os.listdir(DIR)):
        if fn.endswith(".npz"):
            with np.load(os.path.join(DIR, fn)) as f:
                m = json.loads(str(f["meta"]))
            out.append((m["ode"], m["mode"], bool(m["blocked"])))
    return out


_CACHE = {}


def load(shape):
    """The fixture of ``shape`` = (ode, mode, blocked) or its file name without .npz: dict of x[ns, IR], lam[ns, OR], fx[ns, OR],
    jx[ns, OR, IR], gx[ns, IR], hx[ns, IR (IR + 1) / 2] (lower triangle, row-major: (i, j <= i)), the bounds fxE ... hxE (float32,
    rounded upward), IR, OR and meta.  Loaded once; treat as read-only."""
    name = shape if isinstance(shape, str) else shape_name(*shape)
    if name not in _CACHE:
        with np.load(os.path.join(DIR, name + ".npz")) as f:
            d = {k: f[k] for k in f.files}
        d["meta"] = json.loads(str(d["meta"]))
        d["IR"], d["OR"] = d["x"].shape[1], d["lam"].shape[1]
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[name] = d
    return _CACHE[name]


def bound(E, kind):
    return KAPPA[kind] * U * np.asarray(E, dtype=np.float64)


def check(got, fixture, segment_ids, kind, kappa=None):
    """Every entry of ``got[n, ...]`` (no sampling) against fixture segment ``segment_ids[s]`` for row s.  -> dict(worst = the largest
    |got - ref| / bound (inf for a difference at an entry with E = 0), where = (row, flat entry index) of it, over = the number of
    entries over their bound, n = entries compared)."""
    ids = np.asarray(segment_ids, dtype=np.int64)
    ref, E = fixture[kind], fixture[kind + "E"]
    got = np.asarray(got, dtype=np.float64).reshape(ids.size, -1)
    assert got.shape[1] == ref[0].size, (got.shape, ref.shape)
    k = (KAPPA[kind] if kappa is None else kappa) * U
    worst, where, over = 0.0, (0, 0), 0
    for s in np.unique(ids):                                # vectorised over the mesh segments that share a fixture segment
        rows = np.nonzero(ids == s)[0]
        r, b = ref[s].ravel(), k * E[s].ravel().astype(np.float64)
        d = np.abs(got[rows] - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(d == 0.0, 0.0, d / b)              # (b = 0, d > 0: inf;  NaN from the device: stays NaN and counts below)
        bad = ~(q <= 1.0)
        over += int(bad.sum())
        q = np.where(np.isnan(q), np.inf, q)
        m = float(q.max())
        if m > worst:
            i, j = np.unravel_index(int(q.argmax()), q.shape)
            worst, where = m, (int(rows[i]), int(j))
    return dict(worst=worst, where=where, over=over, n=int(got.size))


def block_slots(IR: int, OR: int):
    """Where the fixture's entries sit in a KKT block in the canonical (reference) order ``for i: {H(j, i), j >= i; J(:, i)}``:
    (hslot[IR (IR + 1) / 2] in the fixture's lower-triangle order, jslot[OR, IR])."""
    start = np.zeros(IR, dtype=np.int64)
    for i in range(1, IR):
        start[i] = start[i - 1] + (IR - (i - 1)) + OR
    r, c = np.tril_indices(IR)
    hslot = start[c] + (r - c)
    jslot = (start + (IR - np.arange(IR)))[None, :] + np.arange(OR)[:, None]
    return hslot, jslot


LIBRARY_ODES = ("brachistochrone", "reentry", "twobody_lt", "betts_lowthrust", "synthetic32")


def providers(ode: str):
    """The oracle's derivative providers of an ODE: AD2 for every one, generated analytic derivatives for the library ODEs (the
    run-time compiled families have no generated twin in the oracle)."""
    return ((0, "ad2"), (1, "generated")) if ode in LIBRARY_ODES else ((0, "ad2"),)


def pow2_ceil(x: float) -> float:
    return 2.0 ** math.ceil(math.log2(x))


def oracle_blocks(oracle, fixture, provider):
    """The oracle's (fx, jx, gx, hx lower triangle) of every fixture segment, stacked as the fixture stacks them"""
    m = fixture["meta"]
    ode = oracle.get_ode(m["ode"], provider)
    il = np.tril_indices(fixture["IR"])
    out = [[], [], [], []]
    for s in range(fixture["x"].shape[0]):
        fx, jx, gx, hx = oracle.defect_all(ode, oracle.MODES[m["mode"]], fixture["x"][s], fixture["lam"][s], m["blocked"])
        for o, a in zip(out, (fx, jx, gx, hx[il])):
            o.append(a)
    return dict(zip(KINDS, (np.stack(o) for o in out)))


def measure_constants():
    """dict(worst = {kind: {provider: worst |oracle - ref| / (u E) over every entry of every fixture}}, kappa = {kind: ...},
    inexact = entries with E = 0 the oracle does not reproduce exactly (must be 0))."""
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import bindings as ob
    ob.build()
    worst = {k: {"ad2": 0.0, "generated": 0.0} for k in KINDS}
    at = {k: None for k in KINDS}
    inexact = 0
    for shape in all_shapes():
        f = load(shape)
        ids = np.arange(f["x"].shape[0])
        for prov, pname in providers(shape[0]):
            got = oracle_blocks(ob, f, prov)
            for k in KINDS:
                r = check(got[k], f, ids, k, kappa=1.0)
                if not np.isfinite(r["worst"]):
                    inexact += int(np.sum((f[k + "E"] == 0) & (got[k].reshape(f[k].shape) != f[k])))
                    r = check(np.where(f[k + "E"] == 0, f[k], got[k].reshape(f[k].shape)), f, ids, k, kappa=1.0)
                if r["worst"] > worst[k][pname]:
                    worst[k][pname] = r["worst"]
                    if r["worst"] >= max(worst[k].values()):
                        at[k] = [shape_name(*shape), pname, r["where"][0], r["where"][1]]
    kappa = {k: pow2_ceil(8.0 * max(worst[k].values())) for k in KINDS}
    return dict(worst=worst, at=at, kappa=kappa, inexact=inexact, factor=8.0)
