"""Per-location check of the on-device KKT assembly and of the RHS gathers (tests/test_gpu_assembled_entries.py,
tests/test_assembled_cpu.py).  Pure numpy; nothing under test is touched here.

* The reductions of csrc/capi.hip restated from the kernels' own comments, in float64 and in their order: ``reduce_staged``
  (asm_reduce_kernel: thread t adds cells t, t + 256, ... in sequence from 0.0, then the 256 partial sums are folded by the tree
  w = 128 ... 1), ``gather_short`` (rhs_gather_kernel: one thread adds a row's contributions in source order from 0.0, then adds the
  sum to the target) and ``gather_long`` (rhs_gather_long_kernel: the strided partials and the tree of the staged sums, then target +=).
* Slot-location maps BY CONSTRUCTION (``make_map``): the kernels take slot_locations as given, so a map need not come from a sparsity
  analysis -- it can prescribe how many slots share a location, which of them, where the range starts and which slots are dropped.
* The reference and the bound of a location that takes contributions i = 1 .. k (``sum_reference``): with r_i the 50-digit value of
  contribution i and b_i = defect_checker.bound(E_i, kind) its per-entry bound,

      ref = fsum(r_i)          bound = sum b_i + (k - 1) u sum (|r_i| + b_i)

  The computed contributions c_i are inside b_i of r_i; a float64 sum of k terms IN ANY ORDER is inside (k - 1) u sum |c_i| of their
  exact sum to first order in u (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: every term passes through at
  most k - 1 additions), and |c_i| <= |r_i| + b_i.  For k = 1 nothing is added: the bound is b_1, and with b_1 = 0 the value must be
  exactly the stored one, as in defect_checker.check.  No constant is measured on the device: kappa is defect_checker.KAPPA.
* ``expected_values``: what the default map must leave at every location GIVEN the blocks -- bit for bit wherever the order of the
  additions is fixed or cannot matter.
* ``mult_mesh``: the Mesh of tests/test_gpu_defect_entries.py with a prescribed number of mesh segments per fixture segment.
"""
from __future__ import annotations

import math

import numpy as np

import defect_checker as dc

U = dc.U


# ---- the reductions, restated ------------------------------------------------------------------------------------------------------
def _strided_tree(terms) -> float:
    """256 partial sums -- partial t = ((0.0 + c[t]) + c[t + 256]) + ... -- then part[t] += part[t + w] for w = 128, 64 ... 1."""
    c = np.asarray(terms, dtype=np.float64).ravel()
    rows = -(-c.size // 256)
    padded = np.zeros(max(rows, 1) * 256)                  # (a partial that runs out of cells adds nothing: s + 0.0 == s)
    padded[:c.size] = c
    part = np.zeros(256)
    for row in padded.reshape(-1, 256):                    # one sequential step of every thread at a time
        part = part + row
    w = 128
    while w > 0:
        part[:w] = part[:w] + part[w:2 * w]
        w >>= 1
    return float(part[0])


def reduce_staged(cells) -> float:
    """asm_reduce_kernel: the value a staged location is ASSIGNED, cells in slot order"""
    return _strided_tree(cells)


def gather_short(base: float, terms) -> float:
    """rhs_gather_kernel: base + (((0 + t0) + t1) + ...)"""
    s = 0.0
    for t in np.asarray(terms, dtype=np.float64).ravel():
        s = s + float(t)
    return float(base) + s


def gather_long(base: float, terms) -> float:
    """rhs_gather_long_kernel: base + the strided-and-folded sum"""
    return float(base) + _strided_tree(terms)


SHORT_ROW = 64                                             # rows with more contributors take the long kernel (capi.hip: build_rhs_csr)


def gather(index, blocks, base):
    """The RHS fill restated: target[index[e]] += blocks[e], entries of a row in source order e, short or long by the number of
    contributors.  -> (target, contributors per row)"""
    idx = np.asarray(index).ravel()
    c = np.asarray(blocks, dtype=np.float64).ravel()
    out = np.array(base, dtype=np.float64)
    order = np.argsort(idx, kind="stable")
    rows, start, count = np.unique(idx[order], return_index=True, return_counts=True)
    n = np.zeros(out.size, dtype=np.int64)
    for r, s, k in zip(rows, start, count):
        terms = c[order[s:s + k]]
        out[r] = gather_short(out[r], terms) if k <= SHORT_ROW else gather_long(out[r], terms)
        n[r] = k
    return out, n


# ---- maps by construction --------------------------------------------------------------------------------------------------------------
def hessian_slots(IR: int, OR: int) -> np.ndarray:
    """is_h[NKKT]: which canonical slot is a Hessian entry"""
    hslot, _ = dc.block_slots(IR, OR)
    is_h = np.zeros(IR * (IR + 1) // 2 + OR * IR, dtype=bool)
    is_h[hslot] = True
    return is_h


def make_map(nseg: int, IR: int, OR: int, spec: dict, seed: int):
    """-> (locs[nseg, NKKT] int32, nvalues).  ``spec`` (every key optional):

    hess            sizes of Hessian location classes whose slots are drawn at random over all segments (several of one segment can
                    fall into one class); 2: an atomic pair, >= 3: staged
    hess_distinct   sizes of Hessian classes with ONE slot per segment: class c is block slot hslot[c] of ``size`` random segments
    jac             sizes of Jacobian classes (slots at random over all segments); the string "nseg" stands for nseg
    drop            fraction of all slots marked -1 (none of a hess_distinct class)
    lo              the first location used (default 0);  gaps: unused location numbers inside the range (default 0);
    tail            unused locations behind the range (default 0)

    Every slot that is neither dropped nor in a class has a location of its own.  The location numbers are a random permutation, so
    neither the order of the slots nor Hessian before Jacobian survives; Hessian and Jacobian classes never share a location."""
    rng = np.random.default_rng(seed)
    NK = IR * (IR + 1) // 2 + OR * IR
    hslot, _ = dc.block_slots(IR, OR)
    is_h = np.tile(hessian_slots(IR, OR), nseg)
    free = np.ones(nseg * NK, dtype=bool)
    classes = []
    for c, size in enumerate(spec.get("hess_distinct", ())):
        size = nseg if size == "nseg" else int(size)
        col = np.arange(nseg) * NK + int(hslot[c])
        ids = np.sort(rng.choice(col, size, replace=False))
        free[ids] = False
        classes.append(ids)
    ndrop = int(round(float(spec.get("drop", 0.0)) * free.size))          # (of the slots no one-per-segment class has taken)
    if ndrop:
        free[rng.choice(np.nonzero(free)[0], ndrop, replace=False)] = False
    for pool_is_h, sizes in ((True, spec.get("hess", ())), (False, spec.get("jac", ()))):
        pool = rng.permutation(np.nonzero(free & (is_h == pool_is_h))[0])
        at = 0
        for size in sizes:
            size = nseg if size == "nseg" else int(size)
            assert at + size <= pool.size, "make_map: the classes ask for more slots than there are"
            ids = np.sort(pool[at:at + size])
            at += size
            free[ids] = False
            classes.append(ids)
    singles = np.nonzero(free)[0]
    nloc = len(classes) + singles.size
    lo, gaps = int(spec.get("lo", 0)), int(spec.get("gaps", 0))
    span = nloc + gaps
    assert nloc >= 2
    inner = np.sort(rng.choice(np.arange(1, span - 1), nloc - 2, replace=False)) if gaps else np.arange(1, span - 1)
    numbers = rng.permutation(np.concatenate([[0], inner, [span - 1]])) + lo       # (both ends of the range are used)
    locs = np.full(nseg * NK, -1, dtype=np.int32)
    for ids, m in zip(classes, numbers[:len(classes)]):
        locs[ids] = m
    locs[singles] = numbers[len(classes):]
    return locs.reshape(nseg, NK), lo + span + int(spec.get("tail", 0))


def segment_permuted_map(nseg: int, NK: int, seed: int):
    """Every slot a location of its own, cheap at any size: the segments in reverse order, one random permutation inside every segment."""
    perm = np.random.default_rng(seed).permutation(NK)
    return ((nseg - 1 - np.arange(nseg))[:, None] * NK + perm[None, :]).astype(np.int32), nseg * NK


def intended(nseg: int, IR: int, OR: int, spec: dict) -> dict:
    """What make_map(nseg, IR, OR, spec, .) was asked for, from the spec alone: the sizes of its classes, the slot counts by encoding
    in the default mode, the range."""
    NK = IR * (IR + 1) // 2 + OR * IR
    hs = sorted(nseg if s == "nseg" else int(s) for s in list(spec.get("hess", ())) + list(spec.get("hess_distinct", ())))
    js = sorted(nseg if s == "nseg" else int(s) for s in spec.get("jac", ()))
    dropped = int(round(float(spec.get("drop", 0.0)) * nseg * NK))
    in_classes = sum(hs) + sum(js)
    single = nseg * NK - dropped - in_classes
    lo = int(spec.get("lo", 0))
    return dict(hess=hs, jac=js, dropped=dropped,
                stored=single + sum(s for s in hs + js if s == 1),
                added=sum(s for s in hs if s == 2) + sum(s for s in js if s >= 2),
                staged=sum(s for s in hs if s >= 3), staged_sizes=sorted(s for s in hs if s >= 3),
                lo=lo, hi=lo + len(hs) + len(js) + single + int(spec.get("gaps", 0)))


def classes_of(locs, IR: int, OR: int) -> dict:
    """The classes a map HAS: sorted sizes of the locations Hessian slots name and of those Jacobian slots name (size 1 included),
    dropped slots, and how many locations both kinds name (must be 0)."""
    flat = np.asarray(locs).ravel()
    is_h = np.tile(hessian_slots(IR, OR), flat.size // (IR * (IR + 1) // 2 + OR * IR))
    keep = flat >= 0
    hl, hc = np.unique(flat[keep & is_h], return_counts=True)
    jl, jc = np.unique(flat[keep & ~is_h], return_counts=True)
    return dict(hess=np.sort(hc), jac=np.sort(jc), dropped=int((~keep).sum()), mixed=int(np.intersect1d(hl, jl).size))


# ---- reference and bound of sums of fixture entries ---------------------------------------------------------------------------------
def fixture_blocks(f, pi, hess: bool = True):
    """(r[n, NKKT], b[n, NKKT]): the 50-digit value and the per-entry bound of every KKT slot (canonical order) of a mesh whose
    segment s is fixture segment pi[s].  ``hess`` False: the Jacobian kinds, whose Hessian slots contribute nothing."""
    IR, OR = f["IR"], f["OR"]
    hslot, jslot = dc.block_slots(IR, OR)
    ns = f["x"].shape[0]
    r = np.zeros((ns, IR * (IR + 1) // 2 + OR * IR))
    b = np.zeros_like(r)
    r[:, jslot.ravel()], b[:, jslot.ravel()] = f["jx"].reshape(ns, -1), dc.bound(f["jxE"], "jx").reshape(ns, -1)
    if hess:
        r[:, hslot], b[:, hslot] = f["hx"], dc.bound(f["hxE"], "hx")
    pi = np.asarray(pi, dtype=np.int64)
    return r[pi], b[pi]


def _groups(index, n):
    idx = np.asarray(index).ravel()
    keep = np.nonzero(idx >= 0)[0]
    order = keep[np.argsort(idx[keep], kind="stable")]      # entries of a location in slot / source order
    rows, start, count = np.unique(idx[order], return_index=True, return_counts=True)
    assert rows.size == 0 or rows[-1] < n
    return order, rows, start, count


def sum_parts(index, r, b, n: int):
    """Locations 0 .. n - 1, contribution e goes to index[e] (-1: dropped).  -> (fsum r_i, sum b_i, sum (|r_i| + b_i), count) [n]"""
    r, b = np.asarray(r, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    order, rows, start, count = _groups(index, n)
    ref, sb, sa, cnt = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
    cnt[rows] = count
    one = count == 1
    e = order[start[one]]
    ref[rows[one]], sb[rows[one]], sa[rows[one]] = r[e], b[e], np.abs(r[e]) + b[e]
    for m, s, k in zip(rows[~one], start[~one], count[~one]):
        e = order[s:s + k]
        ref[m], sb[m], sa[m] = math.fsum(r[e]), math.fsum(b[e]), math.fsum(np.abs(r[e]) + b[e])
    return ref, sb, sa, cnt


def sum_reference(index, r, b, n: int):
    """-> (ref[n], bound[n], count[n]) as the module text states"""
    ref, sb, sa, cnt = sum_parts(index, r, b, n)
    return ref, sb + np.maximum(cnt - 1, 0) * U * sa, cnt


def check_sum(got, ref, bnd):
    """-> dict(worst = max |got - ref| / bound (inf: a difference where the bound is 0), where, over, n) as defect_checker.check"""
    got = np.asarray(got, dtype=np.float64)
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0.0, 0.0, d / bnd)
    over = int((~(q <= 1.0)).sum())
    q = np.where(np.isnan(q), np.inf, q)
    return dict(worst=float(q.max()) if q.size else 0.0, where=int(q.argmax()) if q.size else 0, over=over, n=int(got.size))


def expected_values(locs, nvalues: int, blocks, IR: int, OR: int):
    """What the default (not accumulating) map leaves in a zeroed value array, given the blocks [nseg, NKKT] the same kernels produce:
    -> (exp[nvalues], tol[nvalues], count[nvalues], staged[nvalues] bool).  tol == 0: the location is held bit for bit -- one slot
    (the block entry, stored), two slots (fl(a + b): the order of two terms cannot matter), three or more Hessian slots
    (reduce_staged of the cells in slot order).  Three or more Jacobian slots are added atomically in an order nobody knows:
    exp = fsum, tol = (k - 1) u sum |c|.  count == 0: exp = 0 (nothing is written there)."""
    c = np.asarray(blocks, dtype=np.float64).ravel()
    flat = np.asarray(locs).ravel()
    is_h = np.tile(hessian_slots(IR, OR), flat.size // is_h_len(IR, OR))
    order, rows, start, count = _groups(flat, nvalues)
    exp, tol, cnt = np.zeros(nvalues), np.zeros(nvalues), np.zeros(nvalues, dtype=np.int64)
    staged = np.zeros(nvalues, dtype=bool)
    cnt[rows] = count
    one = count == 1
    exp[rows[one]] = c[order[start[one]]]
    two = count == 2
    exp[rows[two]] = c[order[start[two]]] + c[order[start[two] + 1]]
    for m, s, k in zip(rows[count > 2], start[count > 2], count[count > 2]):
        e = order[s:s + k]
        h = is_h[e]
        assert h.all() or not h.any(), "a location both Hessian and Jacobian slots name"
        if h[0]:
            exp[m], staged[m] = reduce_staged(c[e]), True
        else:
            exp[m], tol[m] = math.fsum(c[e]), (k - 1) * U * math.fsum(np.abs(c[e]))
    return exp, tol, cnt, staged


def is_h_len(IR: int, OR: int) -> int:
    return IR * (IR + 1) // 2 + OR * IR


# ---- the constructed maps of the tests: (shape, segments, spec, seed) --------------------------------------------------------------
_J = (1, 2, 2, 3, 3, "nseg")
R7, TB5, B5, S7, C7 = (("reentry", "LGL7", False), ("twobody_lt", "LGL5", True), ("betts_lowthrust", "LGL5", False),
                       ("synthetic32", "LGL7", False), ("coupled12", "LGL7", False))
CONSTRUCTED = [
    # Reentry-LGL7 (528 Hessian slots a segment): many slots of ONE segment in one staged class, sizes at the edges of the reduction
    (R7, 1, dict(hess=(513, 3, 4, 2), jac=_J), 101),
    (R7, 2, dict(hess=(255, 256, 257, 3, 4, 2, 2), jac=_J, drop=0.1), 102),
    (R7, 7, dict(hess=(3, 4, 255, 256, 257, 513, 2, 2, 2), jac=_J, lo=11, gaps=5, tail=3), 103),
    # one contributor per segment, as a phase parameter has
    (R7, 600, dict(hess_distinct=(256, 257, 600), hess=(2, 2), jac=_J), 104),
    (TB5, 7, dict(hess=(3, 4, 5, 2, 2), hess_distinct=("nseg",), jac=_J, drop=0.1), 105),
    (TB5, 300, dict(hess=(3, 257, 2), hess_distinct=(256, "nseg"), jac=_J, lo=17, gaps=9, tail=2), 106),
    (B5, 7, dict(hess=(3, 4, 5, 2, 2), hess_distinct=("nseg",), jac=_J, drop=0.1), 107),
    (B5, 300, dict(hess=(3, 257, 2), hess_distinct=(256, "nseg"), jac=_J, lo=11, gaps=4, tail=1), 108),
    (S7, 7, dict(hess=(3, 4, 513, 2, 2), hess_distinct=("nseg",), jac=_J, drop=0.1), 109),
    (S7, 300, dict(hess=(3, 257, 2), hess_distinct=(256, "nseg"), jac=_J, lo=12, gaps=7), 110),
    (C7, 7, dict(hess=(3, 4, 257, 2, 2), hess_distinct=("nseg",), jac=_J, lo=13, gaps=3, drop=0.1), 111),
]


def constructed_id(case) -> str:
    return f"{dc.shape_name(*case[0])}-x{case[1]}"


def constructed_map(case):
    shape, nseg, spec, seed = case
    f = dc.load(shape)
    return make_map(nseg, f["IR"], f["OR"], spec, seed)


# ---- a mesh with prescribed multiplicities ----------------------------------------------------------------------------------------
def mult_mesh(f, mult, rows: str = "private", seed: int = 3):
    """The Mesh of tests/test_gpu_defect_entries.py in which fixture segment q is named by exactly mult[q] mesh segments (in a random
    order): every variable of q then has mult[q] contributors to AGX.  rows: "private" -- every mesh segment has constraint rows of
    its own (one contributor per row of FXE); "shared" -- the segments that name q share q's rows (mult[q] contributors per row);
    "mixed" -- private, except that the segments of a q with mult[q] >= 256 share the rows of the first of them (many short rows
    AND long rows in one gather)."""
    from test_gpu_defect_entries import Mesh

    class MultMesh(Mesh):
        def __init__(self):
            mu = np.asarray(mult, dtype=np.int64)
            assert mu.size == f["x"].shape[0]
            pi = np.random.default_rng(seed).permutation(np.repeat(np.arange(mu.size), mu))
            super().__init__(f, pi, private_rows=rows != "shared")
            self.mult = mu
            if rows == "mixed":
                cindex = self.cindex.copy()
                for q in np.nonzero(mu >= 256)[0]:
                    segs = np.nonzero(pi == q)[0]
                    cindex[segs] = cindex[segs[0]]          # (L there is lam[q], as for every one of them)
                self.cindex = cindex

    return MultMesh()
