"""The device Krylov drivers on block handles at the vector lengths where the launch geometry of their fused streaming kernels
changes (tests/krylov_edge_problems.py: LENGTHS) and on vectors that are 8-byte but not 16-byte aligned, against the sequential
references tests/test_krylov_edge_problems.py pins on the host.

Every solve runs on a fresh block handle: BlockDiagonalSolver with JacobiLinearSolver() on each block of the 2 x 2 split (two
Jacobi blocks are the monolithic Jacobi, so the references are those of the monolithic matrix).  The first block has an odd size:
inside the library block 1 of every block vector sits at a misaligned offset.  Vector placements per solve:
  (a) numpy host vectors            (b) fresh contiguous device tensors
  (c) x and b both buf[1 : N + 1] of (N + 2)-element device tensors (data_ptr % 16 == 8), guard elements = SENTINEL
  (d) x such a view, b aligned
Per solve: the reference's iteration count and flag, |hist - hist_ref| <= 1e-10 hist[0] (test_gpu_gmres._agree),
max_i |x_i - xref_i| <= 1e-10 max |xref| (element-wise: one wrong element in 1.5e6 fails), b and every guard bit-identical, (a) and
(b) the same bits.  GMRES also with GMG_GMRES_FUSED = 0 on placements (b) and (c): bitwise the fused result."""
import numpy as np
import pytest

import krylov_edge_problems as kp

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77
PLACEMENTS = ("a", "b", "c", "d")
TOL = 1e-10
WORST = {}                                               # (key, N) -> worst element-wise deviation / max|xref| (printed per case)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _solver(S, key, A, N):
    """-> (Krylov solver, the nested block matrix) for one fresh handle"""
    mat = kp.split(A, N)
    nb = len(mat)
    jac = [S.JacobiLinearSolver() for _ in range(nb)]
    kw = kp.tol(key)
    if key == "minres":                                  # Jacobi on diag(|a_ii|): the SPD preconditioner r / |d|
        Pd = S.BlockDiagonalSolver([S.MatrixBlock(D) for D in kp.abs_diag_blocks(A, N)], jac)
        return S.MINRESSolver(Pl=Pd, **kw), mat
    if key == "cg-inner":                                # cg_core on the misaligned sub-vector of block 1
        Pd = S.BlockDiagonalSolver([S.JacobiLinearSolver(), S.CGSolver(S.JacobiLinearSolver(), **kp.INNER_CG)])
        return S.CGSolver(Pd, **kw), mat
    Pd = S.BlockDiagonalSolver(jac)
    if key in ("cg", "fcg"):
        return S.CGSolver(Pd, flexible=(key == "fcg"), **kw), mat
    if key == "fgmres":
        return S.FGMRESSolver(kp.M_GMRES, Pd, restart=True, **kw), mat
    sides = {"gmres-none": dict(Pr=(None, Pd)), "gmres-pr": dict(Pr=Pd), "gmres-pl": dict(Pl=Pd)}[key]
    return S.GMRESSolver(kp.M_GMRES, restart=True, **sides, **kw), mat


def _run(S, key, A, b, N, place):
    """one solve from x = 0 on a fresh handle -> (niters, flag, hist, x)"""
    import torch
    solver, mat = _solver(S, key, A, N)
    ns = S.numerical_setup(S.symbolic_setup(solver, mat), mat)
    try:
        if place == "a":
            x, bh = np.zeros(N), b.copy()
            S.solve_(x, ns, bh)
            assert np.array_equal(_bits(bh), _bits(b)), "b changed"
        else:
            bufs = []

            def view(values):
                buf = torch.full((N + 2,), SENTINEL, dtype=torch.float64, device="cuda")
                v = buf[1:N + 1]
                v.copy_(torch.from_numpy(values))
                assert v.is_contiguous() and v.data_ptr() % 16 == 8
                bufs.append(buf)
                return v

            xd = view(np.zeros(N)) if place in ("c", "d") else torch.zeros(N, dtype=torch.float64, device="cuda")
            bd = view(b) if place == "c" else torch.from_numpy(b).cuda()
            if place in ("b", "d"):
                assert bd.data_ptr() % 16 == 0
            if place == "b":
                assert xd.data_ptr() % 16 == 0
            torch.cuda.synchronize()                     # the library runs on its own stream
            S.solve_(xd, ns, bd)
            torch.cuda.synchronize()
            x = xd.cpu().numpy()
            assert np.array_equal(_bits(bd.cpu().numpy()), _bits(b)), f"placement ({place}): b changed"
            sent = _bits(np.array([SENTINEL]))[0]
            for buf in bufs:
                g = _bits(buf[[0, N + 1]].cpu().numpy())
                assert g[0] == sent and g[1] == sent, f"placement ({place}): a guard element was overwritten: {buf[[0, N + 1]].tolist()}"
        log = solver.log
        return log.num_iters, log.flag, np.array(log.residuals[: log.num_iters + 1]), x
    finally:
        ns.close()


def _agree(key, N, place, got, ref):
    nit, flag, hist, x = got
    xo, nito, flago, histo = ref
    k = min(nit, nito)
    dev = float(np.max(np.abs(x - xo)) / np.max(np.abs(xo)))
    print("%s N=%d (%s): iters %d / %d, flag %d / %d, max |hist - ref| / hist[0] = %.3e, max_i |x_i - xref_i| / max |xref| = %.3e" % (
        key, N, place, nit, nito, flag, flago, np.max(np.abs(hist[: k + 1] - histo[: k + 1])) / histo[0], dev))
    assert (nit, flag) == (nito, flago), (key, N, place, nit, nito, flag, flago)
    assert np.all(np.abs(hist - histo) <= TOL * histo[0]), (key, N, place)
    bad = np.flatnonzero(~(np.abs(x - xo) <= TOL * np.max(np.abs(xo))))
    assert bad.size == 0, (key, N, place, "elements off:", bad[:8].tolist(), x[bad[:8]].tolist(), xo[bad[:8]].tolist())
    WORST[(key, N)] = max(WORST.get((key, N), 0.0), dev)


def _case(S, orc, key, N, monkeypatch=None):
    kind = "spd" if key == "cg-inner" else kp.SOLVERS[key]
    A, b = kp.problem(N, kind)
    ref = kp.reference(key, N, orc)
    got = {}
    for place in PLACEMENTS:
        got[place] = _run(S, key, A, b, N, place)
        _agree(key, N, place, got[place], ref)
    assert got["a"][:2] == got["b"][:2] and np.array_equal(_bits(got["a"][2]), _bits(got["b"][2])) \
        and np.array_equal(_bits(got["a"][3]), _bits(got["b"][3])), "host and device vectors: different bits"
    if monkeypatch is not None:                          # GMRES: the unfused sequence, same operations in the same order
        for place in ("b", "c"):
            monkeypatch.setenv("GMG_GMRES_FUSED", "0")   # a block handle has no option table: read at every solve
            try:
                un = _run(S, key, A, b, N, place)
            finally:
                monkeypatch.delenv("GMG_GMRES_FUSED")
            assert un[:2] == got[place][:2], (key, N, place)
            assert np.array_equal(un[2], got[place][2]), (key, N, place, "history: fused != unfused")
            nd = np.flatnonzero(un[3] != got[place][3])
            assert nd.size == 0 and np.array_equal(un[3], got[place][3]), (key, N, place, "solution: fused != unfused at", nd[:8].tolist())
    print("%s N=%d: %d iterations, worst element-wise deviation %.3e" % (key, N, ref[1], WORST[(key, N)]))


@pytest.mark.parametrize("N", kp.lengths("cg"))
def test_cg_block_jacobi_edge_lengths_and_offsets(S, orc, N):
    _case(S, orc, "cg", N)


@pytest.mark.parametrize("N", kp.lengths("fcg"))
def test_flexible_cg_block_jacobi_edge_lengths_and_offsets(S, orc, N):
    _case(S, orc, "fcg", N)


@pytest.mark.parametrize("N", kp.INNER_CG_LENGTHS)
def test_cg_with_an_inner_cg_on_the_misaligned_block(S, orc, N):
    """block 1 solved by CGSolver(JacobiLinearSolver(), maxiter = 3): cg_core runs on x + n1 with n1 odd"""
    _case(S, orc, "cg-inner", N)


@pytest.mark.parametrize("N", kp.lengths("minres"))
def test_minres_indefinite_abs_jacobi_edge_lengths_and_offsets(S, orc, N):
    _case(S, orc, "minres", N)


@pytest.mark.parametrize("N", kp.lengths("fgmres"))
def test_fgmres_block_jacobi_edge_lengths_and_offsets(S, orc, N):
    _case(S, orc, "fgmres", N)


@pytest.mark.parametrize("N", kp.lengths("gmres-none"))
@pytest.mark.parametrize("form", ["none", "pr", "pl"])
def test_gmres_edge_lengths_and_offsets_fused_and_unfused(S, orc, monkeypatch, form, N):
    """GMRES(10, restart) unpreconditioned (Pr = (None, Pd)), with Pr = Pd and with Pl = Pd"""
    assert kp.lengths("gmres-" + form) == kp.lengths("gmres-none")
    _case(S, orc, "gmres-" + form, N, monkeypatch)
