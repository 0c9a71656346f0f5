"""numpy / scipy restatement of the ChebyshevSmoother on a partitioned level (csrc/cheb.inc.hpp, SEVERAL RANKS).  Plain helper: numpy and
scipy only, no fixtures, no collection hooks.

Everything works on a FOLDED level (halo_edge_problems.case / partition.fold_ranks: the ranks' owned rows stacked in rank order, then
the ghost copies) or on the global matrix in that numbering (gs_dist_reference.folded / folded_hierarchy).

  dinv(L)                          1 / diag of the own x own block: the Jacobi M of the level
  twin_pass(L, co, x, r, M)        one pass on the folded level as the library sums it: z = M(r) ; d = [a d +] b z, each product
                                   rounded, then the sum ; x (+)= d ; r -= (own-column sum in storage order), then -= (ghost-column sum
                                   from 0.0) on the boundary rows -- he.fill / he.ghost_part / oe.seq_spmv, the arithmetic of
                                   gs_dist_reference.twin_pass.  M: "jacobi" or a callable r_own -> z_own
  patch_M(c)                       z = assemble!(local solves of consistent!(r)) of the `patches` family in message order
                                   (he.patch_contributions / he.assemble)
  raw_start / start_vector         the start vector of the estimates: v_i = 1 + ((i * 2654435761) mod 1024)/1024 with i the index among
                                   the rows of ONE handle -- `counts` = [n] for a folded handle (the stacked index), the ranks' owned-row
                                   counts for true ranks -- normalised in the global norm
  power_iteration / lanczos_lambda_max   the two estimates of the setup from a given start vector
  DistCheb                         smoother object of gs_reference.GMG: chebyshev_reference.Cheb with the method and the start vector
                                   as arguments
"""
import math

import numpy as np

import chebyshev_reference as cr
import gs_dist_reference as gd
import halo_edge_problems as he
import operator_edge_problems as oe


def dinv(L):
    return 1.0 / gd.own_block(L).diagonal()


def patch_M(c):
    return lambda r_own: he.assemble(c, he.patch_contributions(c, r_own))


def twin_pass(L, co, x_own, r_own, M="jacobi", x_zero=False):
    """-> (x, r) after one pass of degree len(co[1]) on the folded level L"""
    a, b = co
    S = he._to_scipy(L.A)
    own, gh = he.ghost_part(S, L.n_own)
    bnd = np.diff(gh.indptr) > 0
    q = dinv(L) if isinstance(M, str) else None
    x, r = np.array(x_own, dtype=np.float64), np.array(r_own, dtype=np.float64)
    d = None
    for k in range(b.size):
        z = q * r if q is not None else M(r)
        d = b[0] * z if k == 0 else a[k] * d + b[k] * z       # each product rounded, then the sum
        x = d.copy() if (x_zero and k == 0) else x + d
        v = he.fill(L, d)                                     # consistent!(d)
        r = r - oe.seq_spmv(own, v)                           # own columns, storage order
        r[bnd] = r[bnd] - oe.seq_spmv(gh, v)[bnd]             # the boundary fix-up, mode 1
    return x, r


def raw_start(n):
    i = np.arange(n, dtype=np.uint64)
    return 1.0 + ((i * np.uint64(2654435761)) % np.uint64(1024)).astype(np.float64) / 1024.0


def start_vector(counts):
    """counts: owned rows of every handle, in the order their rows are stacked ([n]: one handle)"""
    v = np.concatenate([raw_start(int(n)) for n in counts])
    return v / np.linalg.norm(v)


def power_iteration(A, M, steps, v0):
    v = np.array(v0, dtype=np.float64)
    lam = None
    for _ in range(steps):
        w = M.solve(A @ v)
        lam = float(np.linalg.norm(w))
        v = w / lam
    return lam


def lanczos_lambda_max(A, M, steps, v0):
    """lanczos_reference.lanczos_tridiagonal from the start vector v0 -> (lambda_est, steps done)"""
    r = np.array(v0, dtype=np.float64)
    gamma_old, gamma0, p = 1.0, None, None
    al, be = [], []
    k = 0
    while k < steps:
        z = M.solve(r)
        gamma = float(z @ r)
        if not (np.isfinite(gamma) and gamma > 0.0):
            break
        if k == 0:
            gamma0 = gamma
        elif gamma < 1e-24 * gamma0:
            break
        beta = gamma / gamma_old
        p = z.copy() if k == 0 else z + beta * p
        w = A @ p
        pw = float(p @ w)
        if not (np.isfinite(pw) and pw > 0.0):
            break
        alpha = gamma / pw
        r = r - alpha * w
        al.append(alpha); be.append(beta)
        gamma_old = gamma
        k += 1
    if k == 0:
        raise np.linalg.LinAlgError("the Lanczos estimate recorded no step")
    T = np.zeros((k, k))
    for i in range(k):
        T[i, i] = 1.0 / al[i] + (be[i] / al[i - 1] if i > 0 else 0.0)
        if i + 1 < k:
            T[i, i + 1] = T[i + 1, i] = math.sqrt(be[i + 1]) / al[i]
    return float(np.linalg.eigvalsh(T).max()), k


def estimate(A, M, method, steps, v0):
    return power_iteration(A, M, steps, v0) if method == "power" else lanczos_lambda_max(A, M, steps, v0)[0]


class DistCheb(cr.Cheb):
    """chebyshev_reference.Cheb on a level of a partitioned handle: eig_method "power" / "lanczos", and the start vector of the
    estimate from `counts` (None: one handle holds all rows of the level -- a folded handle, or a replicated level)"""

    def __init__(self, M, degree=3, eig_method="power", counts=None, **kw):
        super().__init__(M, degree, **kw)
        self.eig_method, self.counts = eig_method, counts

    def setup(self, A):
        M = cr.make_M(self.M, A)
        kw = self.kw
        if kw["lambda_max"] is None:
            est = estimate(A, M, self.eig_method, kw["eig_steps"], start_vector([A.shape[0]] if self.counts is None else self.counts))
            lmax = kw["eig_safety"] * est
        else:
            est, lmax = float("nan"), float(kw["lambda_max"])
        lmin = lmax / kw["eig_ratio"] if kw["lambda_min"] is None else float(kw["lambda_min"])
        return A, M, cr.coefficients(self.degree, lmin, lmax), (est, lmin, lmax)


def gmg_twin(H, levels, specs, degree, eig_method="power", counts=None, cycle="v", **kw):
    """gs_reference.GMG on gs_dist_reference.folded_hierarchy(H, levels) with DistCheb(specs[l], degree) pre and post on level l;
    counts[l]: the handles' owned-row counts of level l (None: one handle) -> (GMG, folded level matrices)"""
    import gs_reference as gr
    mats, Ps, Rs = gd.folded_hierarchy(H, levels)
    po = he._mods()[1]
    w = lambda Ms: [he._po_csr(po, M) for M in Ms]
    sms = [DistCheb(specs[l], degree, eig_method, None if counts is None else counts[l], **kw) for l in range(len(levels) - 1)]
    return gr.GMG(w(mats), w(Ps), w(Rs), sms, sms, cycle=cycle), mats
