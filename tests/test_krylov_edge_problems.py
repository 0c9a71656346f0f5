"""Host checks of the inputs of tests/test_gpu_krylov_edges.py (tests/krylov_edge_problems.py): for every (solver, N) pair the
device file runs, the matrix is what it claims to be and the sequential reference converges by the relative tolerance in a handful
of iterations, with the deciding residuals well away from the threshold -- so the device, whose history agrees to 1e-10 hist[0],
must stop at the same iteration, and a device failure cannot be blamed on the inputs.  No GPU."""
import numpy as np
import pytest

import gmres_reference as gr
import krylov_edge_problems as kp
import numpy_twin as tw

PAIRS = [(key, N) for key in kp.SOLVERS for N in kp.lengths(key)] + [("cg-inner", N) for N in kp.INNER_CG_LENGTHS]


def test_lengths_sit_on_the_launch_geometry_edges():
    """the edges the list claims, from the formulas of csrc/gmg_amd.hip (dot_grid, grid_for, nb of cg_core / minres_core)"""
    dot_grid = lambda n: max(1, min(1024, (n // 2 + 255) // 256))
    grid_for = lambda n: max(1, min(2048, (n + 255) // 256))
    nb = lambda n: max(1, min(1024, (n + 255) // 256))
    trips = lambda elems, grid: -(-elems // (grid * 256))
    assert [dot_grid(n) for n in (511, 512, 513, 514)] == [1, 1, 1, 2]
    assert [dot_grid(n) for n in (131072, 131073, 131074, 131075)] == [256, 256, 257, 257]
    assert [nb(n) for n in (65536, 65537)] == [256, 257]
    assert [trips(n, nb(n)) for n in (262144, 262145)] == [1, 2]
    assert [trips(n, grid_for(n)) for n in (524287, 524288, 524289)] == [1, 1, 2]
    assert [trips(n // 2, dot_grid(n)) for n in (524288, 524289, 524290)] == [1, 1, 2]
    assert [trips(n // 2, grid_for(n)) for n in (1048577, 1048578)] == [1, 2]
    assert trips(1572867, grid_for(1572867)) == 4 and trips(1572867 // 2, dot_grid(1572867)) == 4
    assert dot_grid(523777) == 1023 and dot_grid(523778) == 1024
    for n in (1, 2, 3, 63, 64, 65, 511, 512, 513, 1023, 1024, 65536, 65537, 131072, 131074, 131075, 262144, 262145, 524287, 524288,
              524289, 524290, 1048578, 1572867):
        assert n in kp.LENGTHS
    assert sum(n % 2 == 0 for n in kp.LENGTHS) >= 8 and sum(n % 2 for n in kp.LENGTHS) >= 8
    for key, dropped in kp.DROPPED.items():
        assert set(dropped) <= {1, 2, 3}


@pytest.mark.parametrize("kind", kp.KINDS)
@pytest.mark.parametrize("N", kp.LENGTHS)
def test_matrix_is_what_it_claims(kind, N):
    A, b = kp.problem(N, kind)
    assert A.shape == (N, N) and A.has_sorted_indices and b.shape == (N,) and np.all(b != 0.0) and np.all(np.abs(b) < 1.0)
    A2, b2 = kp.problem(N, kind)
    assert np.array_equal(A.data, A2.data) and np.array_equal(A.indices, A2.indices) and np.array_equal(b, b2)
    D = (A - A.T).tocsr()
    if kind == "nonsym":
        assert N < 2 or abs(D).max() > 0.0
    else:
        assert D.nnz == 0 or abs(D).max() == 0.0
    d = A.diagonal()
    off = np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(d)
    assert np.all(np.abs(d) - off >= 1.0)                                  # Gershgorin: every eigenvalue at modulus >= 1
    assert np.all(np.abs(d) - off <= 2.0 + 1e-12)
    if kind == "indefinite":
        assert np.array_equal(d > 0, (np.arange(N) // 5) % 2 == 0)
    else:
        assert np.all(d > 0)
    want = sorted({0} | {s * k for k in ([1] if N < 9 else [1, N // 3]) if k < N for s in (1, -1)})
    assert sorted(set((A.tocoo().col - A.tocoo().row).tolist())) == want
    blocks = kp.split(A, N)
    if N < 4:
        assert len(blocks) == 1 and blocks[0][0].shape == (N, N)
    else:
        n1 = kp.first_block(N)
        assert n1 % 2 == 1 and 0 < n1 < N
        assert [[m.shape for m in row] for row in blocks] == [[(n1, n1), (n1, N - n1)], [(N - n1, n1), (N - n1, N - n1)]]
        assert blocks[0][1].nnz > 0 and blocks[1][0].nnz > 0
        import scipy.sparse as sp
        K = sp.bmat([[m.to_scipy() for m in row] for row in blocks]).tocsr()
        assert abs(K - A).max() == 0.0
    Dm = kp.abs_diag_blocks(A, N)
    assert np.array_equal(np.concatenate([m.to_scipy().diagonal() for m in Dm]), np.abs(d))


@pytest.mark.parametrize("key,N", PAIRS, ids=lambda v: str(v))
def test_reference_converges_with_margin(orc, key, N):
    x, nit, flag, hist = kp.reference(key, N, orc)
    rtol = kp.tol(key)["rtol"]
    print("%s N=%d: %d iterations, hist[0] = %.6e, last two / (rtol hist[0]) = %.4g %.4g" % (
        key, N, nit, hist[0], hist[-2] / (rtol * hist[0]) if nit else np.nan, hist[-1] / (rtol * hist[0])))
    assert flag == gr.CONVERGED_RTOL
    assert hist.size == nit + 1 and np.all(np.isfinite(hist)) and np.all(np.isfinite(x))
    assert nit <= 60 and (nit >= 3 or N <= 3)
    thr = rtol * hist[0]
    assert hist[nit] < thr and all(h >= thr for h in hist[:nit])
    for h in hist[max(nit - 1, 0):]:
        assert abs(h - thr) >= 0.01 * thr, (key, N, h / thr)              # another seed in kp.SEEDS, never a looser margin
    if N >= 63 and key in ("fgmres", "gmres-none", "gmres-pr", "gmres-pl"):
        assert nit > kp.M_GMRES                                            # at least one restart: the solution update runs twice
    kind = "spd" if key == "cg-inner" else kp.SOLVERS[key]
    A, b = kp.problem(N, kind)
    # it is a solution: hist is the residual in the preconditioner's norm, and |d_i| < 10 (four off-diagonal entries below 1)
    assert np.linalg.norm(A @ x - b) <= 10.0 * rtol * np.linalg.norm(b)


@pytest.mark.parametrize("N", [n for n in kp.SMALL if n <= 1024])
def test_the_numpy_twins_agree_with_the_oracle_drivers(orc, N):
    """numpy_twin.cg(flexible = True) and numpy_twin.fgmres -- independent restatements -- against the oracle's drivers the device
    is compared with: same iteration count, history and solution to rounding"""
    for key, kind in (("fcg", "spd"), ("fgmres", "nonsym")):
        if N not in kp.lengths(key):
            continue
        A, b = kp.problem(N, kind)
        dinv = 1.0 / A.diagonal()
        jac = lambda r: dinv * r
        with np.errstate(all="ignore"):
            if key == "fcg":
                x, nit, hist = tw.cg(A, b.copy(), Pl=jac, flexible=True, **kp.tol(key))
            else:
                x, nit, hist = tw.fgmres(A, b.copy(), Pr=jac, m=kp.M_GMRES, restart=True, **kp.tol(key))
        xo, nito, _, histo = kp.reference(key, N, orc)
        assert nit == nito
        assert np.all(np.abs(hist - histo) <= 1e-10 * histo[0])
        assert np.max(np.abs(x - xo)) <= 1e-10 * np.max(np.abs(xo))
