"""Inputs and references of the patch-smoother edge tests (tests/test_patch_edge_problems.py on the host,
tests/test_gpu_patch_edges.py on the device).  Plain helper, numpy and scipy only: no fixtures, no collection hooks.

level_matrix(family, N, seed)   banded level matrices (half-width 6) whose patch blocks need, or do not need, partial pivoting
two_level(A, agg)               A plus a piecewise-constant coarse level (only level 0's smoother is under test)
patches(N, sizes, seed, mult)   ragged patch sets: whole pairs and singles, scattered, shuffled, with chosen dof multiplicities
periodic_patches(...)           the same on the `periodic` families, where patches of equal shape have bitwise equal blocks
cols_reversed(pp, pd)           the separate column table: every patch's dofs in reverse order
ref_precond / ref_smooth        np.longdouble references; twin_precond / twin_smooth: float64 restatements of the kernels
case(name, kind)                everything one device case needs (cached); reference(name, kind): its references (cached)

The three size regimes of gmg_solver::build_patch / patch_precond (csrc/gmg_amd.hip) the cases are cut for:
  n_p <= 32 (and >= 64 patches)   block de-duplication, patch_apply_dedup_kernel, row-pattern patch operator
  n_p <= 64                       patch_invert_kernel (one wave per patch, [M | X] in LDS) + patch_apply_kernel
  n_p  > 64                       patch_factor_kernel (one thread per patch, global scratch) + patch_apply_big_kernel
"""
import types

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
N_LEVEL = 64 * 31 + 37                                   # 2021 rows: ragged last slice of 64
N_PERIODIC = 64 * 320 + 37                               # 20517 rows: whole CSR operators of >= 20 000 rows are kept in row-pattern form
HALF = 6                                                 # band half-width
PERIOD = 14
OMEGA, NITER = 0.2, 3                                    # Richardson(M, 3, 0.2)
FAMILIES = ("pairs", "dominant", "periodic-pairs", "periodic-dominant")
MULTIPLICITIES = (2, 3, 4, 5, 6, 9)                      # forced on top of 0 (uncovered) and 1: slice widths w with w % 4 = 0, 1, 2, 3

WAVE_SIZES = (1, 2, 3, 17, 31, 32, 33, 47, 62, 63)
DEDUP_SIZES = (1, 2, 5, 16, 31, 32)
BIG_SIZES = (65, 81, 125, 130, 3, 0, 64, 81)


# ------------------------------------------------------------------------------------------------ level matrices
def partner(i, N):
    """the dof paired with i (consecutive pairs inside each group of 7; dofs with i % 7 == 6 and an unpaired last dof are singles)"""
    g = i % 7
    if g == 6:
        return -1
    j = i + 1 if g % 2 == 0 else i - 1
    return j if j < N else -1


def level_matrix(family, N=None, seed=0):
    """-> scipy CSR, sorted.  Band of half-width 6, every entry 0.2 U(-1, 1) except
    "pairs":    a[i, partner] = 4 + U(0, 1), a[i, i] = 0.05 U(0.5, 1) (singles: a[i, i] = 4 + U(0, 1)): partial pivoting swaps
                the two rows of every pair;
    "dominant": a[i, i] = 4 + U(0, 1) on every row: no pivoting needed;
    "periodic-*": the same with every value read from a table indexed by (i mod 14, j - i)."""
    if family not in FAMILIES:
        raise ValueError(family)
    periodic = family.startswith("periodic")
    base = family.split("-")[-1]
    if N is None:
        N = N_PERIODIC if periodic else N_LEVEL
    rng = np.random.default_rng([int(seed), int(N), FAMILIES.index(family)])
    nrow = PERIOD if periodic else N
    W = 2 * HALF + 1
    T = 0.2 * rng.uniform(-1.0, 1.0, (nrow, W))           # T[i, HALF + (j - i)]
    big = 4.0 + rng.uniform(0.0, 1.0, nrow)
    tiny = 0.05 * rng.uniform(0.5, 1.0, nrow)
    for i in range(nrow):
        q = partner(i, PERIOD if periodic else N)
        if base == "dominant" or q < 0:
            T[i, HALF] = big[i]
        else:
            T[i, HALF] = tiny[i]
            T[i, HALF + (q - i)] = big[i]
    i = np.repeat(np.arange(N), W)
    j = i + np.tile(np.arange(-HALF, HALF + 1), N)
    v = T[i % nrow if periodic else i, j - i + HALF]
    keep = (j >= 0) & (j < N)
    A = sp.csr_matrix((v[keep], (i[keep], j[keep])), shape=(N, N))
    A.sort_indices()
    return A


def two_level(A, agg=8):
    """-> dict(mats, prolongations, restrictions) of scipy CSR: piecewise-constant P (agg fine rows per coarse dof), R = P^T,
    A_c = 2 I.  The coarse level only has to exist."""
    N = A.shape[0]
    nH = (N + agg - 1) // agg
    P = sp.csr_matrix((np.ones(N), (np.arange(N), np.arange(N) // agg)), shape=(N, nH))
    P.sort_indices()
    R = P.T.tocsr()
    R.sort_indices()
    Ac = sp.identity(nH, format="csr") * 2.0
    return dict(mats=[A, Ac.tocsr()], prolongations=[P], restrictions=[R])


# ------------------------------------------------------------------------------------------------ patch sets
def units(N):
    """-> (pairs: (npair, 2) array, singles: array); an unpaired last dof belongs to neither"""
    idx = np.arange(N)
    g = idx % 7
    first = idx[(g % 2 == 0) & (g < 6) & (idx + 1 < N)]
    return np.stack([first, first + 1], axis=1), idx[g == 6]


def patches(N, sizes, seed, multiplicities=MULTIPLICITIES):
    """-> (pp int64, pd int32).  Every patch is a union of whole pairs and singles drawn from shuffled pools (so its dofs are
    scattered over the level and interleaved with the other patches'), listed in shuffled order.  For every m of
    `multiplicities` that the set can hold, one pair and (while patches without a single are left) one single sit in exactly m
    patches; every other used dof in one."""
    rng = np.random.default_rng([int(seed), int(N), len(sizes)])
    pr, sg = units(N)
    pr = [u for u in pr[rng.permutation(len(pr))]]
    sg = [np.array([u]) for u in sg[rng.permutation(len(sg))]]
    cap = [int(s) for s in sizes]
    mem = [[] for _ in sizes]
    nsg = [0] * len(cap)                                   # singles per patch: at most 2, so a patch of pairs swaps >= n_p // 2 - 1 rows
    for m in multiplicities:
        for pool in (pr, sg):
            w = pool[-1].size
            cand = [p for p in range(len(cap)) if cap[p] >= w and (w == 2 or nsg[p] == 0)]
            if len(cand) < m:
                continue
            u = pool.pop()
            for p in rng.choice(cand, m, replace=False):
                mem[p].append(u)
                cap[p] -= w
                nsg[p] += w == 1
    for p in range(len(cap)):
        if cap[p] % 2:
            mem[p].append(sg.pop()); cap[p] -= 1
        while cap[p] > 0:
            mem[p].append(pr.pop()); cap[p] -= 2
    pp, pd = [0], []
    for p, us in enumerate(mem):
        d = np.concatenate(us) if us else np.zeros(0, dtype=np.int64)
        d = d[rng.permutation(d.size)]
        if d.size >= 2 and np.all(np.diff(d) > 0):
            d = d[::-1]
        assert d.size == sizes[p] and np.unique(d).size == d.size
        pd.append(d)
        pp.append(pp[-1] + d.size)
    return np.array(pp, dtype=np.int64), np.concatenate(pd).astype(np.int32)


def periodic_patches(N, sizes, npatch, seed, stack=9):
    """-> (pp, pd) on a `periodic` level.  One template per size: every other pair-or-single unit after a base dof (so the dofs are
    not contiguous), an odd size completed by the single 6 dofs after the base, the order shuffled once per size.  Bases are
    multiples of 14 in shuffled order, so patches of one size have bitwise equal blocks, patches that follow one another lie far
    apart, and the windows overlap.  The first `stack` patches of the first size share one base: multiplicity >= stack."""
    rng = np.random.default_rng([int(seed), int(N), int(npatch)])
    tmpl = {}
    for s in sorted(set(sizes)):
        off = []
        if s % 2:
            off.append(6)
        k = 0
        while len(off) < s:                                # pairs at group offsets 0 and 4, then 2 of the next group, ...
            g, u = divmod(k, 2)
            off += [7 * g + (0 if u == 0 else 4), 7 * g + (1 if u == 0 else 5)]
            k += 1
        off = np.array(off, dtype=np.int64)
        assert off.size == s
        tmpl[s] = off[rng.permutation(s)] if s > 1 else off
        if s >= 2 and np.all(np.diff(tmpl[s]) > 0):
            tmpl[s] = tmpl[s][::-1]
    span = max(int(t.max()) for t in tmpl.values() if t.size) + 1
    nbase = (N - span - PERIOD) // PERIOD
    nb = max(npatch // 3, 8)                               # a corner of the level only: the windows of neighbouring bases overlap
    bases = PERIOD * (1 + rng.permutation(nb)[np.arange(npatch) % nb])
    far = PERIOD * (nbase - 2)                             # the stacked patches sit alone at the far end
    pp, pd, seen = [0], [], 0
    for p in range(npatch):
        s = sizes[p % len(sizes)]
        b = bases[p]
        if s == sizes[0] and seen < stack:
            b, seen = far, seen + 1
        pd.append(b + tmpl[s])
        pp.append(pp[-1] + s)
    return np.array(pp, dtype=np.int64), np.concatenate(pd).astype(np.int32)


def cols_reversed(pp, pd):
    pc = pd.copy()
    for p in range(pp.size - 1):
        pc[pp[p]:pp[p + 1]] = pd[pp[p]:pp[p + 1]][::-1]
    return pc


def multiplicity(N, pp, pc):
    return np.bincount(pc[: pp[-1]], minlength=N)


def block(A, rows, cols):
    return A[rows][:, cols].toarray()


def blocks_of(A, pp, rows, cols=None, shift=0.0):
    cols = rows if cols is None else cols
    return [block(A, rows[pp[p]:pp[p + 1]], cols[pp[p]:pp[p + 1]]) + shift * np.eye(int(pp[p + 1] - pp[p])) for p in range(pp.size - 1)]


def pack_colmajor(blocks):
    """the library's patch_mats layout: column-major blocks, concatenated"""
    return np.concatenate([np.asarray(B, dtype=np.float64).reshape(-1, order="F") for B in blocks] + [np.zeros(0)])


# ------------------------------------------------------------------------------------------------ references (np.longdouble)
def _factor(B, pivot):
    """Gaussian elimination of B in np.longdouble; partial pivoting takes the FIRST maximum (pivot = False: plain Doolittle).
    -> (LU, perm, number of row swaps, smallest |pivot|)"""
    M = np.array(B, dtype=LD)
    n = M.shape[0]
    perm = np.arange(n)
    swaps, minpiv = 0, np.inf
    for j in range(n):
        q = j + int(np.argmax(np.abs(M[j:, j]))) if pivot else j
        if q != j:
            M[[j, q]] = M[[q, j]]
            perm[[j, q]] = perm[[q, j]]
            swaps += 1
        d = M[j, j]
        minpiv = min(minpiv, float(abs(d)))
        if d == 0:
            raise ZeroDivisionError("singular block")
        M[j + 1:, j] /= d
        M[j + 1:, j + 1:] -= np.outer(M[j + 1:, j], M[j, j + 1:])
    return M, perm, swaps, minpiv


def _lu_solve(F, b):
    M, perm = F[0], F[1]
    n = M.shape[0]
    y = np.array(b, dtype=LD)[perm]
    for j in range(n):
        y[j + 1:] -= M[j + 1:, j] * y[j]
    for j in range(n - 1, -1, -1):
        y[j] /= M[j, j]
        y[:j] -= M[:j, j] * y[j]
    return y


def ref_factors(A, pp, rows, cols, pivot, blocks=None):
    cols = rows if cols is None else cols
    out = []
    for p in range(pp.size - 1):
        s = slice(pp[p], pp[p + 1])
        B = blocks[p] if blocks is not None else block(A, rows[s], cols[s])
        out.append(_factor(B, pivot))
    return out


def _apply(F, pp, rows, cols, r, N):
    dx = np.zeros(N, dtype=LD)
    for p in range(pp.size - 1):                           # ascending patch order
        s = slice(pp[p], pp[p + 1])
        if s.stop > s.start:
            dx[cols[s]] += _lu_solve(F[p], r[rows[s]])
    return dx


def ref_precond(A, pp, rows, cols, r, pivot, blocks=None, factors=None):
    """x_p = block_p^-1 r[rows_p]; dx[cols_p] += x_p in ascending patch order -> (dx in longdouble, row swaps per patch)"""
    cols = rows if cols is None else cols
    F = factors if factors is not None else ref_factors(A, pp, rows, cols, pivot, blocks)
    return _apply(F, pp, rows, cols, np.asarray(r, dtype=LD), A.shape[0]), np.array([f[2] for f in F], dtype=np.int64)


def _matvec_ld(A, v):
    y = np.zeros(A.shape[0], dtype=LD)
    np.add.at(y, np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), A.data.astype(LD) * v[A.indices])
    return y


def ref_smooth(A, pp, rows, cols, x, r, niter, omega, pivot, blocks=None, factors=None):
    """niter sweeps of dx = omega P r; x += dx; r -= A dx (RichardsonSmoothers.jl:84-98) in longdouble -> (x, r)"""
    cols = rows if cols is None else cols
    F = factors if factors is not None else ref_factors(A, pp, rows, cols, pivot, blocks)
    x, r = np.array(x, dtype=LD), np.array(r, dtype=LD)
    for _ in range(niter):
        dx = LD(omega) * _apply(F, pp, rows, cols, r, A.shape[0])
        x += dx
        r -= _matvec_ld(A, dx)
    return x, r


# ------------------------------------------------------------------------------------------------ float64 twins of the kernels
def twin_inverse(B, pivot, tie_last=False):
    """the explicit row-major inverse as patch_factor_kernel / patch_invert_kernel build it: LU-ordered forward elimination of
    [M | X] (first maximum as pivot, multipliers that are exactly 0 skipped), then back-substitution on every column of X.
    tie_last: the LAST of equal maxima instead -- the wrong tie rule, to show that the bits tell the two apart"""
    M = np.array(B, dtype=np.float64)
    n = M.shape[0]
    X = np.eye(n)
    for j in range(n):
        col = np.abs(M[j:, j])
        q = (j + (int(np.argmax(col)) if not tie_last else col.size - 1 - int(np.argmax(col[::-1])))) if pivot else j
        if q != j:
            M[[j, q]] = M[[q, j]]
            X[[j, q]] = X[[q, j]]
        d = M[j, j]
        if d == 0.0:
            raise ZeroDivisionError("singular block")
        l = M[j + 1:, j] / d
        M[j + 1:, j + 1:] -= l[:, None] * M[j, j + 1:][None, :]
        X[j + 1:] -= l[:, None] * X[j][None, :]
        M[j + 1:, j] = 0.0
    for j in range(n - 1, -1, -1):
        s = X[j].copy()
        for k in range(j + 1, n):
            s -= M[j, k] * X[k]
        X[j] = s / M[j, j]
    return X


def twin_inverses(A, pp, rows, cols, pivot, blocks=None):
    cols = rows if cols is None else cols
    return [twin_inverse(blocks[p] if blocks is not None else block(A, rows[pp[p]:pp[p + 1]], cols[pp[p]:pp[p + 1]]), pivot)
            for p in range(pp.size - 1)]


def _twin_apply(X, pp, rows, cols, r, N):
    dx = np.zeros(N)
    for p in range(pp.size - 1):
        s = slice(pp[p], pp[p + 1])
        b = r[rows[s]]
        c = np.zeros(b.size)
        for k in range(b.size):                            # row . vector, summed in column order
            c += X[p][:, k] * b[k]
        dx[cols[s]] += c                                   # ascending-patch sums (a dof appears once per patch)
    return dx


def twin_precond(A, pp, rows, cols, r, pivot, blocks=None, inverses=None):
    cols = rows if cols is None else cols
    X = inverses if inverses is not None else twin_inverses(A, pp, rows, cols, pivot, blocks)
    return _twin_apply(X, pp, rows, cols, np.asarray(r, dtype=np.float64), A.shape[0])


def twin_smooth(A, pp, rows, cols, x, r, niter, omega, pivot, blocks=None, inverses=None):
    cols = rows if cols is None else cols
    X = inverses if inverses is not None else twin_inverses(A, pp, rows, cols, pivot, blocks)
    x, r = np.array(x, dtype=np.float64), np.array(r, dtype=np.float64)
    for _ in range(niter):
        dx = omega * _twin_apply(X, pp, rows, cols, r, A.shape[0])
        x = x + dx
        r = r - A @ dx
    return x, r


def max_rel(a, b):
    """max|a - b| / max|b| (conftest.max_rel) in the precision of the arguments"""
    m = np.max(np.abs(b))
    d = np.max(np.abs(a - b))
    return float(d / m) if m > 0 else float(d)


# ------------------------------------------------------------------------------------------------ cases
# name -> the kinds it runs under ("lu": PatchSolver, "nopivot": BlockJacobiSolver); which family, patch set, column table and
# caller blocks a name stands for is decided in case()
CASES = {
    "wave63": dict(kinds=("lu", "nopivot")),
    "wave64": dict(kinds=("lu", "nopivot")),
    "dedup_ragged": dict(kinds=("lu", "nopivot")),
    "big": dict(kinds=("lu", "nopivot")),
    "big_cols": dict(kinds=("lu",)),
    "wave_cols": dict(kinds=("lu",)),
    "dense": dict(kinds=("lu",)),
    "sell_refresh": dict(kinds=("lu", "nopivot")),          # wave63 patches on the second draw of the family
    "sell_refresh_big": dict(kinds=("lu", "nopivot")),      # big patches on the second draw
}
CASE_KEYS = [(name, kind) for name, c in CASES.items() for kind in c["kinds"]]


def wave_sizes(npatch=43, with64=False):
    s = [WAVE_SIZES[p % len(WAVE_SIZES)] for p in range(npatch)]
    if with64:
        s[len(WAVE_SIZES) + 8] = 64                        # one 64-dof patch (in place of a 62): max_np == 64
    return s


_CASE, _REF, _TWIN = {}, {}, {}


def case(name, kind):
    """-> namespace(A, N, agg, pp, pd, pc (None: cols = rows), pivot, blocks (None: A[rows_p, cols_p]), r, x0).  Shared: read only."""
    if (name, kind) in _CASE:
        return _CASE[(name, kind)]
    if kind not in CASES[name]["kinds"]:
        raise ValueError((name, kind))
    pivot = kind == "lu"
    fam = "pairs" if pivot else "dominant"
    seed, agg, pc, blocks = 0, 8, None, None
    if name in ("big_cols", "wave_cols"):
        fam = "dominant"
    if name.startswith("sell_refresh"):
        seed = 1                                           # the second draw: what update_values hands over
    if name == "dedup_ragged":
        fam, agg = "periodic-" + fam, 64
    A = level_matrix(fam, seed=seed)
    N = A.shape[0]
    if name in ("wave63", "sell_refresh"):
        pp, pd = patches(N, wave_sizes(), 11)
    elif name in ("wave64", "wave_cols", "dense"):
        pp, pd = patches(N, wave_sizes(with64=True), 12)
    elif name in ("big", "big_cols", "sell_refresh_big"):
        pp, pd = patches(N, BIG_SIZES, 13)
    else:
        pp, pd = periodic_patches(N, DEDUP_SIZES, 64 * 3 + 9, 14)
    if name in ("big_cols", "wave_cols"):
        pc = cols_reversed(pp, pd)
    if name == "dense":
        blocks = blocks_of(A, pp, pd, shift=0.5)
    rng = np.random.default_rng([99, len(name), int(pivot)])
    c = types.SimpleNamespace(name=name, kind=kind, family=fam, seed=seed, A=A, N=N, agg=agg, pp=pp, pd=pd, pc=pc, pivot=pivot,
                              blocks=blocks, r=rng.uniform(-1.0, 1.0, N), x0=rng.uniform(-1.0, 1.0, N))
    for a in (c.pp, c.pd, c.r, c.x0) + ((c.pc,) if pc is not None else ()):
        a.setflags(write=False)
    _CASE[(name, kind)] = c
    return c


def reference(name, kind):
    """-> namespace(dx, x, r as float64 roundings of the longdouble results, dx_ld, x_ld, r_ld, swaps, minpiv)"""
    if (name, kind) in _REF:
        return _REF[(name, kind)]
    c = case(name, kind)
    F = ref_factors(c.A, c.pp, c.pd, c.pc, c.pivot, c.blocks)
    dx, swaps = ref_precond(c.A, c.pp, c.pd, c.pc, c.r, c.pivot, factors=F)
    x, r = ref_smooth(c.A, c.pp, c.pd, c.pc, c.x0, c.r, NITER, OMEGA, c.pivot, factors=F)
    out = types.SimpleNamespace(dx_ld=dx, x_ld=x, r_ld=r, dx=dx.astype(np.float64), x=x.astype(np.float64), r=r.astype(np.float64),
                                swaps=swaps, minpiv=np.array([f[3] for f in F]))
    for a in vars(out).values():
        a.setflags(write=False)
    _REF[(name, kind)] = out
    return out


def twin(name, kind):
    if (name, kind) in _TWIN:
        return _TWIN[(name, kind)]
    c = case(name, kind)
    X = twin_inverses(c.A, c.pp, c.pd, c.pc, c.pivot, c.blocks)
    dx = twin_precond(c.A, c.pp, c.pd, c.pc, c.r, c.pivot, inverses=X)
    x, r = twin_smooth(c.A, c.pp, c.pd, c.pc, c.x0, c.r, NITER, OMEGA, c.pivot, inverses=X)
    _TWIN[(name, kind)] = (dx, x, r)
    return _TWIN[(name, kind)]


# ------------------------------------------------------------------------------------------------ ad-hoc cases (caller blocks)
def adhoc_case(name, A, pp, pd, blocks, pivot, seed=5):
    """a case namespace like case()'s for a test that brings its own patch set and caller blocks"""
    rng = np.random.default_rng([int(seed), len(name)])
    N = A.shape[0]
    return types.SimpleNamespace(name=name, kind="lu" if pivot else "nopivot", family="adhoc", seed=seed, A=A, N=N, agg=8, pp=pp, pd=pd,
                                 pc=None, pivot=pivot, blocks=blocks, r=rng.uniform(-1.0, 1.0, N), x0=rng.uniform(-1.0, 1.0, N))


def adhoc_reference(c):
    F = ref_factors(c.A, c.pp, c.pd, c.pc, c.pivot, c.blocks)
    dx, swaps = ref_precond(c.A, c.pp, c.pd, c.pc, c.r, c.pivot, factors=F)
    x, r = ref_smooth(c.A, c.pp, c.pd, c.pc, c.x0, c.r, NITER, OMEGA, c.pivot, factors=F)
    return types.SimpleNamespace(dx_ld=dx, x_ld=x, r_ld=r, dx=dx.astype(np.float64), x=x.astype(np.float64), r=r.astype(np.float64),
                                 swaps=swaps, perms=[f[1] for f in F], minpiv=np.array([f[3] for f in F]))


def antidiagonal_case(pivot):
    """five small patches of `dominant` with caller blocks A[p, p] + 0.5 I, block 2 replaced by [[0, 1], [1, 0]]"""
    A = level_matrix("dominant")
    pp, pd = patches(A.shape[0], (2, 2, 2, 3, 2), 21, multiplicities=(2,))
    blocks = blocks_of(A, pp, pd, shift=0.5)
    blocks[2] = np.array([[0.0, 1.0], [1.0, 0.0]])
    return adhoc_case("antidiagonal", A, pp, pd, blocks, pivot)


TIE_ROWS = ((0, (0, 17, 32), (5.0, 5.0, -5.0)), (1, (5, 20), (6.0, -6.0)))


def tie_case():
    """Equal column maxima (LU, caller blocks, every dof in one patch): in the 33-dof block of three patches of `dominant`
    column 0 holds |5| in rows 0, 17 and 32 -- the first maximum is the diagonal, no swap -- and column 1 holds |6| in rows 5 and
    20 over a diagonal of 0.1 -- the first maximum is row 5, one swap.  Rows 17 / 32 and 5 / 20 sit in different halves of every
    butterfly stage of patch_invert_kernel's argmax.  Any choice among equal maxima solves the system; only the bits differ."""
    A = level_matrix("dominant")
    pp, pd = patches(A.shape[0], (33, 5, 2), 31, multiplicities=())
    blocks = blocks_of(A, pp, pd, shift=0.5)
    B = blocks[0]
    for colj, rows, vals in TIE_ROWS:
        for r, v in zip(rows, vals):
            B[r, colj] = v
    B[1, 1], B[1, 5], B[5, 5] = 0.1, 5.0, 0.0              # rows 1 and 5 form a pair: after the swap both pivots are large
    B[5, 0] = B[20, 0] = 0.0                                # rows 5 and 20 go through the elimination of column 0 untouched
    return adhoc_case("tie", A, pp, pd, blocks, True)
