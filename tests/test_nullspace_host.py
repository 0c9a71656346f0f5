"""Host checks of the null-space feature (no GPU): the reference's own main_interfaces() cases (test/LinearSolvers/NullspaceTests.jl:
13-35) against tests/nullspace_reference.py, the argument checks of NullSpace / NullspaceSolver that need no device, the Neumann
hierarchy generator, and the invariance the GPU test of the projection relies on (the kernel component of the iterate of a Krylov
method on a symmetric singular matrix with a consistent right-hand side never changes)."""
import numpy as np
import pytest

import gmres_reference as gr
import nullspace_reference as nr


def test_reference_main_interfaces_nullspace_of_a_matrix():
    """NullspaceTests.jl:14-25"""
    A = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    V = nr.nullspace_of_matrix(A)
    assert len(V) == 2
    assert nr.is_orthonormal(V)                                                  # :17
    assert nr.is_orthogonal(V, np.array([1.0, 0.0, 0.0]))                        # :18
    assert not nr.is_orthogonal(V, np.array([0.0, 1.0, 0.0]))                    # :19
    v = np.array([1.0, 2.0, 3.0])
    p, alpha = nr.project(V, v)                                                  # :22
    w, beta = nr.make_orthogonal_(V, v.copy())                                   # :23
    u = nr.reconstruct(V, w, alpha)                                              # :24
    assert np.allclose(u, v, rtol=np.sqrt(np.finfo(float).eps), atol=0.0)        # :25 (isapprox)
    assert np.allclose(p + w, v) and np.allclose(alpha, beta)                    # orthonormal basis: both give the same coefficients
    assert nr.is_orthogonal(V, A=lambda x: A @ x)


def test_reference_main_interfaces_gram_schmidt_variants_agree():
    """NullspaceTests.jl:27-34"""
    V1 = [np.array(v) for v in ([2.0, 1.0, 1.0], [1.0, 2.0, 1.0], [1.0, 1.0, 1.0])]
    nr.gram_schmidt_(V1)
    assert nr.is_orthonormal(V1)                                                 # :29
    V2 = [np.array(v) for v in ([2.0, 1.0, 1.0], [1.0, 2.0, 1.0], [1.0, 1.0, 1.0])]
    nr.modified_gram_schmidt_(V2)
    assert nr.is_orthonormal(V2)
    assert np.allclose(np.stack(V1), np.stack(V2), rtol=np.sqrt(np.finfo(float).eps), atol=0.0)   # :34


def test_nullspace_constructor_and_accessors(S):
    N = S.NullSpace([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    assert N.size() == (2, 3) and N.size(0) == 2 and N.size(1) == 3              # NullSpaces.jl:13-14
    assert N.matrix_representation().shape == (3, 2)                             # stack(N.V), :17-19
    assert np.array_equal(N.matrix_representation()[:, 1], [4.0, 5.0, 6.0])
    assert S.NullSpace(N.matrix_representation()).size() == (2, 3)               # n x k array: its columns
    assert S.NullSpace(np.ones(7)).size() == (1, 7)                              # :21
    assert S.NullSpace([1.0, 1.0, 1.0]).size() == (1, 3)
    M = N.merge(S.NullSpace(np.ones(3)))                                         # :15
    assert M.size() == (3, 3) and np.array_equal(M.V[2], np.ones(3))
    with pytest.raises(ValueError, match="same length"):                         # @assert :7
        S.NullSpace([np.ones(3), np.ones(4)])
    A = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    Nm = S.NullSpace.from_matrix(A)                                              # :23-26
    ref = nr.nullspace_of_matrix(A)
    assert Nm.size() == (2, 3) and all(np.array_equal(a, b) for a, b in zip(Nm.V, ref))
    with pytest.raises(ValueError, match="trivial"):
        S.NullSpace.from_matrix(np.eye(3))


def test_unbound_nullspace_raises_a_clear_error(S):
    N = S.NullSpace(np.ones(5))
    v = np.ones(5)
    for call in (lambda: S.project(N, v), lambda: S.project_(np.zeros(5), N, v), lambda: S.make_orthogonal_(N, v),
                 lambda: S.reconstruct(N, v, [1.0]), lambda: S.reconstruct_(N, v, [1.0]), lambda: S.is_orthonormal(N),
                 lambda: S.is_orthogonal(N), lambda: S.is_orthogonal(N, v), lambda: S.make_orthonormal_(N),
                 lambda: S.gram_schmidt_(N), lambda: S.modified_gram_schmidt_(N)):
        with pytest.raises(RuntimeError, match="bind"):
            call()
    with pytest.raises(ValueError, match="Unknown method"):                      # NullSpaces.jl:73
        S.make_orthonormal_(N, method="householder")


def test_nullspace_solver_argument_checks(S, po):
    H = po.neumann_hierarchy((4, 4), 2)
    n, nL = H["mats"][0].shape[0], H["mats"][1].shape[0]
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], coarsest_solver=S.CGSolver(S.JacobiLinearSolver()))
    N = S.NullSpace(np.ones(n))
    s = S.NullspaceSolver(S.GMRESSolver(10, Pr=(None, gmg)), N)
    assert s.constrain_matrix is True                                            # the reference's default, NullspaceSolvers.jl:38
    with pytest.raises(NotImplementedError, match="projected mode"):             # no top-level direct solver on the device
        S.symbolic_setup(s)
    with pytest.raises(NotImplementedError, match="projected mode"):
        S.symbolic_setup(S.NullspaceSolver(S.LUSolver(), N))
    with pytest.raises(TypeError):
        S.NullspaceSolver(S.GMRESSolver(10, Pr=(None, gmg)), np.ones(n))
    with pytest.raises(TypeError):
        S.NullspaceSolver(gmg, N)
    with pytest.raises(NotImplementedError, match="Krylov"):
        S.symbolic_setup(S.NullspaceSolver(S.LUSolver(), N, constrain_matrix=False))
    ss = S.symbolic_setup(S.NullspaceSolver(S.GMRESSolver(10, Pr=(None, gmg)), N, constrain_matrix=False))
    assert ss.solver.nullspace is N
    # the coarsest slot of a GMG takes NullspaceSolver(LUSolver(), N_coarse) and nothing else of that kind
    S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], coarsest_solver=S.NullspaceSolver(S.LUSolver(), S.NullSpace(np.ones(nL))))
    with pytest.raises(NotImplementedError):
        S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"],
                          coarsest_solver=S.NullspaceSolver(S.LUSolver(), S.NullSpace(np.ones(nL)), constrain_matrix=False))
    with pytest.raises(NotImplementedError):
        S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"],
                          coarsest_solver=S.NullspaceSolver(S.CGSolver(S.JacobiLinearSolver()), S.NullSpace(np.ones(nL))))
    with pytest.raises(ValueError, match="coarsest matrix"):
        S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], coarsest_solver=S.NullspaceSolver(S.LUSolver(), N))


@pytest.mark.parametrize("nc,nlev,order", [((4, 4), 2, 1), ((8, 8), 3, 1), ((4, 4, 4), 2, 1), ((4, 4), 2, 2)])
def test_neumann_hierarchy_kernel_transfers_and_rhs(po, nc, nlev, order):
    H = po.neumann_hierarchy(nc, nlev, order)
    assert len(H["mats"]) == nlev and len(H["prolongations"]) == nlev - 1
    for l, A in enumerate(H["mats"]):
        As = A.to_scipy()
        n = As.shape[0]
        assert n == int(np.prod([order * c + 1 for c in H["ncells"][l]]))        # every node is a dof
        assert abs(As - As.T).max() == 0.0
        normA = np.sqrt((As.data ** 2).sum())
        assert np.linalg.norm(As @ np.ones(n)) <= 1e-12 * normA                  # the constants are in the kernel ...
        ev = np.linalg.eigvalsh(As.toarray())
        assert ev[0] > -1e-12 * ev[-1] and ev[1] > 1e-6 * ev[-1]                 # ... and nothing else is: semi-definite, one zero
    for l, P in enumerate(H["prolongations"]):
        Ps = P.to_scipy()
        assert Ps.shape == (H["mats"][l].shape[0], H["mats"][l + 1].shape[0])
        assert np.array_equal(Ps @ np.ones(Ps.shape[1]), np.ones(Ps.shape[0]))   # P 1_H = 1_h
        assert abs(H["restrictions"][l].to_scipy() - Ps.T).max() == 0.0          # R = P'
    b = po.neumann_rhs(nc, order)
    assert b.size == H["mats"][0].shape[0] and np.linalg.norm(b) > 0.1
    assert abs(b.sum()) <= 1e-12 * np.linalg.norm(b) * np.sqrt(b.size)           # b is orthogonal to the kernel: consistent system
    with pytest.raises(ValueError):
        po.neumann_hierarchy((6, 6), 3)


def test_existing_dirichlet_generators_are_untouched(po):
    """the new functions share the 1-D tables with the Dirichlet ones: interior block of the Neumann matrix == poisson_matrix"""
    nc = (4, 6)
    An = po.neumann_matrix(nc).to_scipy().toarray().reshape(7, 5, 7, 5)
    Ad = po.poisson_matrix(nc).to_scipy().toarray()
    assert np.array_equal(An[1:-1, 1:-1, 1:-1, 1:-1].reshape(Ad.shape), Ad)


def test_constrained_and_projected_restatements_on_the_reference_problem(po):
    """NullspaceTests.jl:39-81 on the host: both modes solve the Neumann problem and return x orthogonal to the constants; and the
    invariance the GPU test uses -- without the projection the kernel component of the guess stays in the iterate."""
    nc = (4, 4)
    A = po.neumann_matrix(nc).to_scipy().tocsr()
    Ad = A.toarray()
    n = A.shape[0]
    b = po.neumann_rhs(nc)
    V = [np.ones(n)]
    assert np.linalg.norm(Ad @ np.stack(V, axis=1)) < 1e-10                      # :60
    x = nr.solve_constrained(Ad, V, b)                                           # :63-68
    assert np.linalg.norm(A @ x - b) < 1e-10 and abs(x @ V[0]) < 1e-10           # :69-70
    nr.gram_schmidt_(V)                                                          # make_orthonormal!(N), NullspaceSolvers.jl:68
    x0 = np.random.default_rng(7).standard_normal(n)
    inner = lambda g, rhs: gr.gmres(lambda u: A @ u, rhs, 10, x0=g, rtol=1e-12, givens=_givens)
    xs, nit, flag, hist = nr.solve_projected(V, x0, b, inner)                    # :73-78
    assert flag in (gr.CONVERGED_ATOL, gr.CONVERGED_RTOL)
    assert np.linalg.norm(A @ xs - b) < 1e-10 and abs(xs @ V[0]) < 1e-10         # :79-80
    xu, _n, _f, _h = inner(x0, b)                                                # no projection
    assert np.linalg.norm(A @ xu - b) < 1e-10
    assert abs(xu @ V[0] - x0 @ V[0]) < 1e-8 and abs(x0 @ V[0]) > 1e-3           # the component is still there


def _givens(f, g):
    """LinearAlgebra.givensAlgorithm for the well-scaled numbers of this file (no oracle build needed on the host)"""
    if g == 0.0:
        return 1.0, 0.0, f
    if f == 0.0:
        return 0.0, 1.0, g
    r = float(np.hypot(f, g))
    c, s = f / r, g / r
    if abs(f) > abs(g) and c < 0.0:
        c, s, r = -c, -s, -r
    return c, s, r
