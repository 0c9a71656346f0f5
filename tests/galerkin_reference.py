"""Numpy twin of the Galerkin coarse matrices (tests only): the two-stage ordered product of include/gmg_amd.h, gmg_set_galerkin,

    T = A P        T(i, J) = sum over k ascending of A(i, k) * P(k, J)
    A_c = R T    A_c(I, J) = sum over i ascending of R(I, i) * T(i, J)

every sum from 0.0, every product and every sum rounded separately (Python floats: IEEE double, no contraction), only stored entries
contribute, the patterns are the structural products, columns ascend in every row.  Plain loops over Python lists.

Also the ragged and the cancelling test problems the host and the GPU tests share.
"""
import numpy as np


class M:
    """0-based CSR: shape, ptr (int64), idx (int32), val -- the fields solvers._csr_fields reads"""

    def __init__(self, shape, ptr, idx, val):
        self.shape = (int(shape[0]), int(shape[1]))
        self.ptr = np.ascontiguousarray(ptr, dtype=np.int64)
        self.idx = np.ascontiguousarray(idx, dtype=np.int32)
        self.val = np.ascontiguousarray(val, dtype=np.float64)

    def to_scipy(self):
        import scipy.sparse as sp
        return sp.csr_matrix((self.val, self.idx, self.ptr), shape=self.shape)


def sorted_rows(A):
    """the same matrix with ascending columns in every row (stable; the stored operator is not touched)"""
    ptr, idx, val = A.ptr, A.idx.copy(), A.val.copy()
    for i in range(A.shape[0]):
        k0, k1 = ptr[i], ptr[i + 1]
        o = np.argsort(idx[k0:k1], kind="stable")
        idx[k0:k1] = idx[k0:k1][o]
        val[k0:k1] = val[k0:k1][o]
    return M(A.shape, ptr, idx, val)


def transpose(P):
    """P^T with ascending columns, entry values unchanged"""
    n, m = P.shape
    cnt = np.zeros(m + 1, dtype=np.int64)
    np.add.at(cnt, P.idx.astype(np.int64) + 1, 1)
    ptr = np.cumsum(cnt)
    fill = ptr[:-1].copy()
    idx, val = np.empty(P.idx.size, dtype=np.int32), np.empty(P.idx.size)
    for i in range(n):
        for k in range(P.ptr[i], P.ptr[i + 1]):
            q = fill[P.idx[k]]
            fill[P.idx[k]] += 1
            idx[q] = i
            val[q] = P.val[k]
    return M((m, n), ptr, idx, val)


def product(A, B):
    """C = A B with the ordered sums above; A and B with ascending columns"""
    aptr, aidx, aval = A.ptr.tolist(), A.idx.tolist(), A.val.tolist()
    bptr, bidx, bval = B.ptr.tolist(), B.idx.tolist(), B.val.tolist()
    ptr, idx, val = [0], [], []
    for i in range(A.shape[0]):
        acc = {}
        for k in range(aptr[i], aptr[i + 1]):
            a, r = aval[k], aidx[k]
            for q in range(bptr[r], bptr[r + 1]):
                J = bidx[q]
                acc[J] = acc.get(J, 0.0) + a * bval[q]
        cols = sorted(acc)
        idx.extend(cols)
        val.extend(acc[J] for J in cols)
        ptr.append(len(idx))
    return M((A.shape[0], B.shape[1]), ptr, idx, val)


def galerkin(R, A, P):
    """-> (T, A_c); R = None means P^T.  Inputs with unsorted rows are sorted in copies."""
    A, P = sorted_rows(A), sorted_rows(P)
    R = transpose(P) if R is None else sorted_rows(R)
    T = product(A, P)
    return T, product(R, T)


def chain(A0, Ps, Rs=None):
    """[A0, R0 A0 P0, R1 (R0 A0 P0) P1, ...]: a hierarchy whose levels 1.. are all Galerkin"""
    mats = [A0]
    for l, P in enumerate(Ps):
        mats.append(galerkin(None if Rs is None or Rs[l] is None else Rs[l], mats[-1], P)[1])
    return mats


# ---- shared test problems ----------------------------------------------------------------------------------------------------------
def ragged_problem(seed, nf=61, nc=23):
    """Rectangular P (nf x nc) with rows of 0 .. 5 entries and every column non-empty; R = a perturbed P^T (same pattern, other values,
    plus a few extra entries); nonsymmetric diagonally dominant A with unsorted rows and one explicit zero.  Rows 0 and 1 of P and row 0
    of T = A P have no entries."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(nf):
        k = int(rng.integers(0, 6))
        rows.append(sorted(rng.choice(nc, size=k, replace=False).tolist()))
    rows[0] = rows[1] = []                                    # rows without entries, always
    for J in range(nc):                                       # every column non-empty
        if not any(J in r for r in rows):
            i = 2 + int(rng.integers(0, nf - 2))
            while len(rows[i]) >= 5:
                i = 2 + ((i - 1) % (nf - 2))
            rows[i] = sorted(rows[i] + [J])
    pptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    pidx = np.array([c for r in rows for c in r], dtype=np.int32)
    P = M((nf, nc), pptr, pidx, rng.uniform(0.2, 1.0, pidx.size))
    Pt = transpose(P)
    rrows = []
    for I in range(nc):
        cols = Pt.idx[Pt.ptr[I]:Pt.ptr[I + 1]].tolist()
        extra = [int(c) for c in rng.choice(nf, size=2, replace=False) if int(c) not in cols]
        rrows.append(sorted(cols + extra))
    rptr = np.concatenate([[0], np.cumsum([len(r) for r in rrows])])
    ridx = np.array([c for r in rrows for c in r], dtype=np.int32)
    R = M((nc, nf), rptr, ridx, rng.uniform(0.2, 1.0, ridx.size))
    arows, avals = [], []
    for i in range(nf):
        off = [int(c) for c in rng.choice(nf, size=int(rng.integers(1, 6)), replace=False) if int(c) != i]
        if i == 0:
            off = [1]                                         # row 0 of A meets the empty rows 0 and 1 of P only: T(0, :) has no entries
        cols = [i] + off
        vals = [10.0 + float(rng.uniform(0.0, 1.0))] + [float(v) for v in rng.uniform(-1.0, 1.0, len(off))]
        if i == 5 and off:
            vals[1] = 0.0                                     # the explicit zero
        o = rng.permutation(len(cols))                        # unsorted rows
        arows.append([cols[j] for j in o])
        avals.append([vals[j] for j in o])
    aptr = np.concatenate([[0], np.cumsum([len(r) for r in arows])])
    A = M((nf, nf), aptr, [c for r in arows for c in r], [v for r in avals for v in r])
    return dict(A=A, P=P, R=R)


RAGGED_SEED = 3    # cond(R A P) of the twin's product is below 1e8 with this seed (asserted in tests/test_galerkin_host.py)


def cancelling_problem():
    """Terms that cancel in both stages: T(1, 1) = 2*1 + (-2)*1 and A_c(1, 0) = 1*3 + 1*(-3) stay stored 0.0 (R = P^T); the coarse
    matrix [[7.5, -1], [0, 1]] stays regular."""
    P = M((4, 2), [0, 1, 3, 4, 5], [0, 0, 1, 1, 0], [1.0, 1.0, 1.0, 1.0, 0.5])
    A = M((4, 4), [0, 2, 5, 7, 9], [0, 1, 0, 1, 2, 1, 2, 0, 3], [4.0, -1.0, 1.0, 2.0, -2.0, -3.0, 4.0, 0.5, 5.0])
    return dict(A=A, P=P, R=None)
