"""Matrix families and Krylov cases of the Gauss-Seidel smoother tests (tests/test_gs_host.py on the host,
tests/test_gpu_gauss_seidel.py on the device).  Plain helper: no fixtures, no collection hooks, nothing read from outside the
repository.  Every family comes wrapped into a two-level hierarchy the way operator_edge_problems.case() wraps its own (ragged
P and R, a given SPD coarse matrix); the synthetic families carry a full nonzero diagonal, a diagonally dominant form and
off-diagonal magnitudes 1e-3 .. 1e3 (operator_edge_problems.square_matrix).

family       rows        what it is there for
q1_3d-0/-1   3375, 343   levels 0 and 1 of hierarchy((16,16,16), 3): 27-point rows; 99 and 43 sets, largest 60 and 14 rows
q1_2d        3969        level 0 of hierarchy((64,64), 3): 9-point; 187 sets, largest 32
q2_3d        3375        level 0 of hierarchy((8,8,8), 2, order=2): up to 125 entries per row; 183 sets, largest 30
redblack     4096        5-point Laplacian on a 64 x 64 node grid, red nodes first: two sets of 2048 rows each way -> wide launches only
diagonal     2500        one set, one wide launch, no off-diagonal entry
bidiagonal   300         lower: forward 300 sets of one row, backward one set of 300
tridiagonal  2000        2000 sets of one row each way: the longest barrier chain
blocks       5320        row blocks of BLOCK_SIZES; the sets are exactly the blocks; 1024 stays in a chain, 1025 goes wide
shuffled     5320        `blocks` with the entries of every row stored in a random order
one_row      1           n = 1
diagonal_big 528609      (device test only) one set; more rows than one pass of the capped grid of the x += dx launch covers
no_diag / zero_diag      q1_2d with one diagonal entry removed / set to 0: GMG_ERR_SINGULAR
"""
import functools
import types

import numpy as np
import scipy.sparse as sp

import __graft_entry__ as entry
import operator_edge_problems as oe

BLOCK_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 5, 1)
POISSON = ("q1_3d-0", "q1_3d-1", "q1_2d", "q2_3d")
FAMILIES = POISSON + ("redblack", "diagonal", "bidiagonal", "tridiagonal", "blocks", "shuffled", "one_row")
SINGULAR = ("no_diag", "zero_diag")
BAD_ROW = 1234                       # the row of q1_2d whose diagonal entry no_diag drops / zero_diag zeroes
BIG_ROWS = 2048 * 256 + 4321         # `diagonal_big`: more rows than the element-wise launches' capped grid (2048 x 256) has threads

# (sets, rows of the largest set) forward = backward on these families; launches and wide launches follow from gs_reference.launch_plan
SETS = {"q1_3d-0": (99, 60), "q1_3d-1": (43, 14), "q1_2d": (187, 32), "q2_3d": (183, 30), "redblack": (2, 2048),
        "diagonal": (1, 2500), "tridiagonal": (2000, 1), "blocks": (10, 2049), "shuffled": (10, 2049), "one_row": (1, 1)}
SETS_BIDIAGONAL = {True: (300, 1), False: (1, 300)}
# (launches, wide launches) per direction
PLANS = {"blocks": (4, 2), "redblack": (2, 2), "diagonal": (1, 1), "q1_3d-0": (1, 0), "q1_3d-1": (1, 0)}


def _po():
    return entry.import_package().poisson


def _sorted_csr(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M


@functools.lru_cache(maxsize=None)
def _poisson_level(nc, nlev, order, lev):
    return _sorted_csr(_po().build_hierarchy(nc, nlev, order)["mats"][lev].to_scipy())


def _redblack(m=64):
    i, j = np.divmod(np.arange(m * m), m)
    red = (i + j) % 2 == 0
    number = np.empty(m * m, dtype=np.int64)
    number[red] = np.arange(np.count_nonzero(red))
    number[~red] = np.count_nonzero(red) + np.arange(np.count_nonzero(~red))
    rows, cols, vals = [number], [number], [np.full(m * m, 4.0)]
    for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        ok = (i + di >= 0) & (i + di < m) & (j + dj >= 0) & (j + dj < m)
        rows.append(number[ok]); cols.append(number[(i + di)[ok] * m + (j + dj)[ok]]); vals.append(np.full(np.count_nonzero(ok), -1.0))
    return _sorted_csr(sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(m * m, m * m)))


def _block_rows():
    """rows of the `blocks` structure: every row of block k > 0 has 1-6 lower entries, at least one of them in block k - 1, every row
    of block k < 9 has 1-6 upper entries, at least one in block k + 1; no other entry inside the row's own block than the diagonal"""
    rng = oe._rng(7, sum(BLOCK_SIZES), 3)
    start = np.concatenate([[0], np.cumsum(BLOCK_SIZES)])
    rows = []
    for k, size in enumerate(BLOCK_SIZES):
        for i in range(start[k], start[k + 1]):
            c = [i]
            if k > 0:
                c.append(int(rng.integers(start[k - 1], start[k])))
                c.extend(int(q) for q in rng.integers(0, start[k], int(rng.integers(0, 6))))
            if k < len(BLOCK_SIZES) - 1:
                c.append(int(rng.integers(start[k + 1], start[k + 2])))
                c.extend(int(q) for q in rng.integers(start[k + 1], start[-1], int(rng.integers(0, 6))))
            rows.append(np.unique(np.array(c, dtype=np.int64)))
    return rows


def _shuffle_rows(A, seed=11):
    """the same matrix with the entries of every row stored in a random order (raw CSR, never re-sorted)"""
    rng = oe._rng(seed, A.shape[0], 4)
    idx, val = A.indices.copy(), A.data.copy()
    for i in range(A.shape[0]):
        a, b = A.indptr[i], A.indptr[i + 1]
        p = rng.permutation(b - a)
        idx[a:b], val[a:b] = A.indices[a:b][p], A.data[a:b][p]
    return oe._csr(val, idx, A.indptr, A.shape)


def _drop_entry(A, row, col):
    keep = np.ones(A.nnz, dtype=bool)
    k = A.indptr[row] + int(np.flatnonzero(A.indices[A.indptr[row]:A.indptr[row + 1]] == col)[0])
    keep[k] = False
    ptr = A.indptr.copy()
    ptr[row + 1:] -= 1
    return oe._csr(A.data[keep], A.indices[keep], ptr, A.shape)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """-> scipy CSR (rows sorted, except `shuffled`)"""
    if name == "q1_3d-0":
        return _poisson_level((16, 16, 16), 3, 1, 0)
    if name == "q1_3d-1":
        return _poisson_level((16, 16, 16), 3, 1, 1)
    if name == "q1_2d":
        return _poisson_level((64, 64), 3, 1, 0)
    if name == "q2_3d":
        return _poisson_level((8, 8, 8), 2, 2, 0)
    if name == "redblack":
        return _redblack()
    if name == "diagonal":
        rng = oe._rng(2500, 9)
        return _sorted_csr(sp.diags(rng.choice([-1.0, 1.0], 2500) * 10.0 ** rng.uniform(-3.0, 3.0, 2500)))
    if name == "diagonal_big":
        rng = oe._rng(BIG_ROWS, 9)
        return _sorted_csr(sp.diags(rng.choice([-1.0, 1.0], BIG_ROWS) * 10.0 ** rng.uniform(-3.0, 3.0, BIG_ROWS)))
    if name == "bidiagonal":
        return oe.square_matrix([np.arange(max(i - 1, 0), i + 1) for i in range(300)])
    if name == "tridiagonal":
        return oe.square_matrix([np.arange(max(i - 1, 0), min(i + 2, 2000)) for i in range(2000)])
    if name == "blocks":
        return oe.square_matrix(_block_rows())
    if name == "shuffled":
        return _shuffle_rows(matrix("blocks"))
    if name == "one_row":
        return oe._csr([2.5], [0], [0, 1], (1, 1))
    if name == "no_diag":
        return _drop_entry(matrix("q1_2d"), BAD_ROW, BAD_ROW)
    if name == "zero_diag":
        A = matrix("q1_2d").copy()
        A.data[A.indptr[BAD_ROW] + int(np.flatnonzero(A.indices[A.indptr[BAD_ROW]:A.indptr[BAD_ROW + 1]] == BAD_ROW)[0])] = 0.0
        return oe._csr(A.data, A.indices, A.indptr, A.shape)
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> namespace(name, A, P, R, Ac, n, nH, x0, r0): the family's matrix as the fine level of a two-level hierarchy"""
    A = matrix(name)
    n = A.shape[0]
    nH = oe.coarse_size(n)
    if name == "diagonal_big":                                # (the ragged generators draw row by row: an aggregation here)
        v = oe._rng(n, nH, 14).uniform(0.25, 1.0, n)
        P = _sorted_csr(sp.csr_matrix((v, (np.arange(n), np.arange(n) % nH)), shape=(n, nH)))
        R = _sorted_csr(P.T)
    else:
        P = oe.rect_matrix(oe.tall_ragged(n, nH), nH)
        R = oe.rect_matrix(oe.wide_ragged(nH, n), n)
    absum = lambda M: float(np.mean(np.abs(M).sum(axis=1))) or 1.0
    Ac = oe.coarse_matrix(nH, float(np.mean(np.abs(A.diagonal()))) * absum(P) * absum(R))
    rng = oe._rng((FAMILIES + SINGULAR + ("diagonal_big",)).index(name), n, 13)
    return types.SimpleNamespace(name=name, A=A, P=P, R=R, Ac=Ac, n=n, nH=nH, x0=rng.uniform(-1, 1, n), r0=rng.uniform(-1, 1, n))


# ------------------------------------------------------------------------------------------------ Krylov cases
# smoothers: ("gs", niter, omega, type) or ("rj", niter, omega).  rhs = dirichlet_lift_rhs(nc, 1), x0 = 0.  `iters` is the iteration
# count of the numpy reference (tests/test_gs_host.py asserts it, and that the relative residual one iteration before the end is
# at least 1.5 rtol and the last one at most rtol / 1.5: no count sits on an edge).
SYM5 = ("gs", 5, 1.0, "symmetric")
SYM1 = ("gs", 1, 1.0, "symmetric")
FWD2 = ("gs", 2, 0.9, "forward")
RJ3 = ("rj", 3, 2.0 / 3.0)
KRYLOV = {
    # the reference's own test, SmoothersTests.jl:46-56: CG + LinearSolverFromSmoother(SymGS(5)) as the two-level GMG's finest pre-smoother
    "smoother-2d": dict(nc=(8, 8), nlev=2, pre=SYM5, post=SYM5, solver="cg_smoother", cycle="v", rtol=1e-8, iters=4),
    "smoother-3d": dict(nc=(8, 8, 8), nlev=2, pre=SYM5, post=SYM5, solver="cg_smoother", cycle="v", rtol=1e-8, iters=4),
    "cg-2d-sym": dict(nc=(32, 32), nlev=3, pre=SYM1, post=SYM1, solver="cg", cycle="v", rtol=1e-8, iters=5),
    "cg-3d-mixed": dict(nc=(16, 16, 16), nlev=3, pre=RJ3, post=SYM1, solver="cg", cycle="v", rtol=1e-8, iters=5),
    "fgmres-3d-fwd": dict(nc=(16, 16, 16), nlev=3, pre=FWD2, post=FWD2, solver="fgmres", cycle="v", rtol=1e-8, iters=5),
    "cg-2d-wcycle": dict(nc=(32, 32), nlev=3, pre=SYM1, post=SYM1, solver="cg", cycle="w", rtol=1e-8, iters=3),
    "gmg-solver-2d": dict(nc=(32, 32), nlev=3, pre=SYM1, post=SYM1, solver="gmg", cycle="v", rtol=1e-8, iters=6),
}


def reference_smoother(spec):
    import gs_reference as gr
    return gr.GS(*spec[1:]) if spec[0] == "gs" else gr.RJ(*spec[1:])


@functools.lru_cache(maxsize=None)
def krylov_reference(name):
    """the numpy reference of one Krylov case -> (x, iterations, residual history)"""
    import gs_reference as gr
    c = KRYLOV[name]
    po = _po()
    H = po.build_hierarchy(c["nc"], c["nlev"], 1)
    b = po.dirichlet_lift_rhs(c["nc"], 1)
    A = _sorted_csr(H["mats"][0].to_scipy())
    pre, post = reference_smoother(c["pre"]), reference_smoother(c["post"])
    G = gr.GMG(H["mats"], H["prolongations"], H["restrictions"], [pre] * (c["nlev"] - 1), [post] * (c["nlev"] - 1), cycle=c["cycle"])
    kw = dict(maxiter=100, atol=1e-14, rtol=c["rtol"])
    if c["solver"] == "cg_smoother":
        ns = pre.setup(A)
        return gr.cg(A, b, Pl=lambda r: gr.ldiv(ns, pre, r), **kw)
    if c["solver"] == "cg":
        return gr.cg(A, b, Pl=G.solve, **kw)
    if c["solver"] == "fgmres":
        return gr.fgmres(A, b, Pr=G.solve, m=5, **kw)
    return G.solver(b, **kw)
