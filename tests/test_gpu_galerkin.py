"""Galerkin coarse matrices on the device (csrc/galerkin.inc.hpp, kernels.hpp galerkin_gather_kernel) against the numpy twin
(tests/galerkin_reference.py).

1. bits: level_matrix == the twin, pattern and values
2. equivalence: a handle with Galerkin levels and a handle given level_matrix(l) through gmg_set_matrix
3. a large level: the finest matrix in row-pattern form, 20 449 coarse rows
4. solves: iteration counts and x
5. refresh: update(A') against a fresh setup
6. refusals"""
import ctypes as C
import functools

import numpy as np
import pytest

import galerkin_reference as gal
import numpy_twin as nt

pytestmark = pytest.mark.gpu

TOL = 1e-13     # the project's per-kernel bound: max|a - b| / max|b|


def _jacobi(S, nlev):
    return [S.RichardsonSmoother(S.JacobiLinearSolver(), 10, 2.0 / 3.0) for _ in range(nlev - 1)]


def _ns(S, mats, Ps, Rs, sm=None, options=None, **kw):
    sm = _jacobi(S, len(mats)) if sm is None else sm
    kw.setdefault("maxiter", 1)
    g = S.GMGLinearSolver(mats, Ps, Rs, pre_smoothers=sm, post_smoothers=sm, options=options, **kw)
    return S.numerical_setup(S.symbolic_setup(g, mats[0]), mats[0])


def _galerkin_ns(S, A0, Ps, Rs, sm=None, options=None, **kw):
    return _ns(S, [A0] + [S.Galerkin() for _ in Ps], Ps, Rs, sm, options, **kw)


def _equal(ns, lev, want):
    shape, ptr, idx, val = ns.level_matrix(lev)
    assert shape == want.shape and ptr.dtype == np.int64 and idx.dtype == np.int32
    assert np.array_equal(ptr, want.ptr) and np.array_equal(idx, want.idx), f"pattern of level {lev}"
    assert np.array_equal(val, want.val), f"values of level {lev}: max diff {np.max(np.abs(val - want.val)):.3e}"


def _level_csr(po, ns, lev):
    shape, ptr, idx, val = ns.level_matrix(lev)
    return po.CSR(shape, ptr, idx, val)


@functools.lru_cache(maxsize=None)
def _problem(name):
    """-> (A0, Ps, Rs, twin matrices of every level); computed once, shared and left unchanged"""
    import __graft_entry__ as entry
    po = entry.import_package().poisson
    if name == "ragged":
        c = gal.ragged_problem(gal.RAGGED_SEED)
        A0, Ps, Rs = c["A"], [c["P"]], [c["R"]]
    elif name == "cancelling":
        c = gal.cancelling_problem()
        A0, Ps, Rs = c["A"], [c["P"]], None
    else:
        nc, nlev, order, kappa = {"q1_8x3": ((8, 8, 8), 3, 1, None), "q1_8x3_kappa": ((8, 8, 8), 3, 1, po.smooth_kappa),
                                  "q2_8x2": ((8, 8), 3, 2, None), "q2_8x3": ((8, 8, 8), 2, 2, None),
                                  "q1_32x2": ((32, 32), 3, 1, None), "q1_16x3": ((16, 16, 16), 3, 1, None),
                                  "q2_16x2": ((16, 16), 3, 2, None)}[name]
        H = po.build_hierarchy(nc, nlev, order, kappa=kappa)
        A0, Ps, Rs = H["mats"][0], H["prolongations"], H["restrictions"]
    return A0, Ps, Rs, gal.chain(A0, Ps, Rs)


# ---------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("name,options", (("q1_8x3", None), ("q1_8x3_kappa", None), ("q2_8x2", None), ("q2_8x3", None),
                                          ("ragged", None), ("cancelling", None), ("q2_8x2", {"force_ptr64": 1})))
def test_level_matrix_bits(S, name, options):
    """chains of two Galerkin levels, rows of up to 125 entries (Q2 8^3), rows without entries and unsorted input rows (ragged),
    entries that cancel to a stored 0.0; 32- and 64-bit row pointers"""
    A0, Ps, Rs, twin = _problem(name)
    if name == "q2_8x3":
        assert np.diff(twin[1].ptr).max() == 125
    if name == "cancelling":
        assert twin[1].val[2] == 0.0
    ns = _galerkin_ns(S, A0, Ps, Rs, options=options)
    try:
        for l in range(1, len(twin)):
            _equal(ns, l, twin[l])
        assert ns.sizes == [m.shape[0] for m in twin]
    finally:
        ns.close()


# ---------------------------------------------------------------- 2. equivalence with the same matrices handed over
@pytest.mark.parametrize("name,options", (("q1_8x3", None), ("q2_8x2", None), ("q1_32x2", {"eager_min_rows": 200})))
def test_same_as_a_handle_given_the_matrices(S, po, pkg, name, options):
    """(eager_min_rows = 200: levels 0 and 1 of Q1 32^2 are kept in row-pattern form -- the finer level's rows come back out of the
    stream, the Galerkin level itself takes the eager conversion)"""
    A0, Ps, Rs, twin = _problem(name)
    nlev = len(twin)
    ng = _galerkin_ns(S, A0, Ps, Rs, options=options)
    nm = None
    try:
        for l in range(1, nlev):
            _equal(ng, l, twin[l])
        nm = _ns(S, [A0] + [_level_csr(po, ng, l) for l in range(1, nlev)], Ps, Rs, options=options)
        b = np.random.default_rng(11).standard_normal(A0.shape[0])
        xg, xm = np.zeros_like(b), np.zeros_like(b)
        S.solve_(xg, ng, b)
        S.solve_(xm, nm, b)
        assert np.array_equal(xg, xm) and np.all(np.isfinite(xg)) and np.linalg.norm(xg) > 0
        for l in range(nlev):
            assert ng.level_format(l) == nm.level_format(l)
            assert ng.sweep_signature(l) == nm.sweep_signature(l)
        if options:
            assert ng.level_format(1)["row_patterns"] and ng.level_format(0)["row_patterns"]
        assert ng.device_bytes() == nm.device_bytes()
        with pytest.raises(pkg.abi.GmgError):
            nm.level_matrix(1)                                # not a Galerkin level
    finally:
        ng.close()
        if nm is not None:
            nm.close()


# ---------------------------------------------------------------- 3. a large level
def test_large_level(S, po, hierarchy):
    """Q1 288^2, 2 levels: the finest matrix (83 521 rows) is kept in row-pattern form by gmg_set_matrix and gives its rows back for
    the product; level 1 has 20 449 rows"""
    H = hierarchy((288, 288), 2, 1)
    A0, Ps, Rs = H["mats"][0], H["prolongations"], H["restrictions"]
    ng = _galerkin_ns(S, A0, Ps, Rs)
    nr = None
    try:
        shape, ptr, idx, val = ng.level_matrix(1)
        assert shape == (20449, 20449)
        Sp = (Rs[0].to_scipy() @ (A0.to_scipy() @ Ps[0].to_scipy())).tocsr()
        got = po.CSR(shape, ptr, idx, val).to_scipy()
        err = abs(got - Sp).max() / np.max(np.abs(Sp.data))
        print(f"large level: max|device - scipy| / max|scipy| = {err:.3e}")
        assert err <= TOL
        red = H["mats"][1].to_scipy().tocsr()
        red.sort_indices()
        assert np.array_equal(ptr, red.indptr) and np.array_equal(idx, red.indices)      # the pattern of the re-discretised matrix
        nr = _ns(S, H["mats"], Ps, Rs)
        assert ng.level_format(1) == nr.level_format(1)
        b = np.random.default_rng(11).standard_normal(A0.shape[0])
        xg, xr = np.zeros_like(b), np.zeros_like(b)
        S.solve_(xg, ng, b)
        S.solve_(xr, nr, b)
        assert ng.level_format(0) == nr.level_format(0) and ng.level_format(0)["row_patterns"]
        assert ng.sweep_signature(0) == nr.sweep_signature(0)
        assert np.all(np.isfinite(xg)) and np.all(np.isfinite(xr))
    finally:
        ng.close()
        if nr is not None:
            nr.close()


# ---------------------------------------------------------------- 4. solves
def _device_cg(S, mats, Ps, Rs, b):
    sm = _jacobi(S, len(mats))
    g = S.GMGLinearSolver(mats, Ps, Rs, pre_smoothers=sm, post_smoothers=sm, maxiter=1)
    cg = S.CGSolver(g, maxiter=50, atol=1e-14, rtol=1e-8)
    ns = S.numerical_setup(S.symbolic_setup(cg, mats[0]), mats[0])
    try:
        x = np.zeros_like(b)
        S.solve_(x, ns, b)
        return cg.log.num_iters, x
    finally:
        ns.close()


@pytest.mark.parametrize("name,iters", (("q1_16x3", 3), ("q2_16x2", 4)))
def test_cg_solves(S, po, hierarchy, name, iters):
    """CG + GMG(Jacobi 10, 2/3), rtol 1e-8"""
    A0, Ps, Rs, twin = _problem(name)
    nc, order = {"q1_16x3": ((16, 16, 16), 1), "q2_16x2": ((16, 16), 2)}[name]
    H = hierarchy(nc, 3, order)
    b = np.random.default_rng(5).standard_normal(A0.shape[0])
    it_g, x_g = _device_cg(S, [A0, S.Galerkin(), S.Galerkin()], Ps, Rs, b)
    it_r, x_r = _device_cg(S, H["mats"], Ps, Rs, b)
    jac = [(nt.Jacobi(m.to_scipy().tocsr()), 10, 2.0 / 3.0) for m in twin[:-1]]
    tw = nt.GMG(twin, Ps, Rs, jac)
    x_t, it_t, _hist = nt.cg(A0.to_scipy().tocsr(), b, Pl=tw.solve, maxiter=50, atol=1e-14, rtol=1e-8)
    print(f"{name}: iterations Galerkin {it_g}, re-discretised {it_r}, twin {it_t}")
    assert it_g == it_r == it_t == iters
    e_t, e_r = np.linalg.norm(x_g - x_t) / np.linalg.norm(x_t), np.linalg.norm(x_g - x_r) / np.linalg.norm(x_r)
    print(f"{name}: |x - twin| = {e_t:.3e}, |x - re-discretised| = {e_r:.3e} (relative)")
    assert e_t <= 1e-10 and e_r <= 1e-10


def test_fgmres_patch_solve(S, po, hierarchy):
    """FGMRES(5) + GMG(RichardsonSmoother(PatchSolver, 10, 0.2)) on Q2 8^2, 3 levels"""
    A0, Ps, Rs, twin = _problem("q2_8x2")
    H = hierarchy((8, 8), 3, 2)
    tabs = [po.vertex_star_patches(c, 2) for c in H["ncells"][:2]]
    b = np.random.default_rng(5).standard_normal(A0.shape[0])

    def device(mats):
        sm = [S.RichardsonSmoother(S.PatchSolver(pp, pd), 10, 0.2) for pp, pd in tabs]
        g = S.GMGLinearSolver(mats, Ps, Rs, pre_smoothers=sm, post_smoothers=sm, maxiter=1)
        fg = S.FGMRESSolver(5, g, maxiter=50, atol=1e-14, rtol=1e-8)
        ns = S.numerical_setup(S.symbolic_setup(fg, mats[0]), mats[0])
        try:
            x = np.zeros_like(b)
            S.solve_(x, ns, b)
            return fg.log.num_iters, x
        finally:
            ns.close()

    it_g, x_g = device([A0, S.Galerkin(), S.Galerkin()])
    it_r, x_r = device(H["mats"])
    pat = [(nt.Patch(m.to_scipy().tocsr(), pp, pd), 10, 0.2) for m, (pp, pd) in zip(twin[:-1], tabs)]
    tw = nt.GMG(twin, Ps, Rs, pat)
    x_t, it_t, _hist = nt.fgmres(A0.to_scipy().tocsr(), b, Pr=tw.solve, m=5, maxiter=50, atol=1e-14, rtol=1e-8)
    print(f"fgmres + patch: iterations Galerkin {it_g}, re-discretised {it_r}, twin {it_t}")
    assert it_g == it_r == it_t
    e_t, e_r = np.linalg.norm(x_g - x_t) / np.linalg.norm(x_t), np.linalg.norm(x_g - x_r) / np.linalg.norm(x_r)
    print(f"fgmres + patch: |x - twin| = {e_t:.3e}, |x - re-discretised| = {e_r:.3e} (relative)")
    assert e_t <= 1e-10 and e_r <= 1e-10


# ---------------------------------------------------------------- 5. refresh
@pytest.mark.parametrize("smoother", ("jacobi", "pmult"))
def test_update_matches_a_fresh_setup(S, po, smoother):
    """smooth_kappa Q1 16^3, 3 levels: update(A') with the values of another coefficient, twice"""
    nc, nlev = (16, 16, 16), 3
    H = po.build_hierarchy(nc, nlev, 1, kappa=po.smooth_kappa)
    A0, Ps, Rs = H["mats"][0], H["prolongations"], H["restrictions"]
    others = [po.poisson_matrix_varcoef(nc, lambda X, Y, Z, s=s: po.smooth_kappa(X, Y, Z) * (1.0 + s * X * Y + 0.5 * s * Z)) for s in (0.3, 0.7)]
    for Ap in others:
        assert np.array_equal(Ap.ptr, A0.ptr) and np.array_equal(Ap.idx, A0.idx) and not np.array_equal(Ap.val, A0.val)

    def smoothers():
        if smoother == "jacobi":
            return _jacobi(S, nlev)
        return [S.MultiplicativePatchSmoother(S.PatchSolver(*po.vertex_star_patches(c, 1))) for c in H["ncells"][:2]]

    def setup(A):
        sm = smoothers()
        g = S.GMGLinearSolver([A, S.Galerkin(), S.Galerkin()], Ps, Rs, pre_smoothers=sm, post_smoothers=sm, maxiter=1)
        cg = S.CGSolver(g, maxiter=50, atol=1e-14, rtol=1e-8)
        return cg, S.numerical_setup(S.symbolic_setup(cg, A), A)

    def observe(cg, ns):
        b = np.random.default_rng(5).standard_normal(A0.shape[0])
        x = np.zeros_like(b)
        S.solve_(x, ns, b)
        g = ns.P_ns
        out = dict(x=x, iters=cg.log.num_iters, mats=[g.level_matrix(l) for l in (1, 2)],
                   fmt=[g.level_format(l) for l in range(nlev)], sig=[g.sweep_signature(l) for l in range(nlev)])
        if smoother == "pmult":
            out["colors"] = [g.patch_coloring(l) for l in range(nlev - 1)]
        return out

    cg, ns = setup(A0)
    try:
        first = observe(cg, ns)
        for Ap in others:
            S.numerical_setup_(ns, Ap)
            got = observe(cg, ns)
            cg_f, ns_f = setup(Ap)
            try:
                want = observe(cg_f, ns_f)
            finally:
                ns_f.close()
            for (s1, p1, i1, v1), (s2, p2, i2, v2) in zip(got["mats"], want["mats"]):
                assert s1 == s2 and np.array_equal(p1, p2) and np.array_equal(i1, i2) and np.array_equal(v1, v2)
            assert not np.array_equal(got["mats"][0][3], first["mats"][0][3])             # the values did change
            assert np.array_equal(got["x"], want["x"]) and got["iters"] == want["iters"]
            assert got["fmt"] == want["fmt"] == first["fmt"] and got["sig"] == want["sig"]
            if smoother == "pmult":
                for (n1, c1), (n2, c2), (n0, c0) in zip(got["colors"], want["colors"], first["colors"]):
                    assert n1 == n2 == n0 and np.array_equal(c1, c2) and np.array_equal(c1, c0)
    finally:
        ns.close()


# ---------------------------------------------------------------- 6. refusals
def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_refusals_of_the_entry_points(S, po, pkg):
    """level 0 and levels out of range, value updates of a Galerkin level, the accessor on other levels and with small arrays: the
    code, the level in the message, and the handle solves as before"""
    abi = pkg.abi
    A0, Ps, Rs, twin = _problem("q1_8x3")
    ns = _ns(S, [A0, S.Galerkin(), twin[2]], Ps, Rs)
    lib, h = ns._lib, ns.h
    try:
        b = np.random.default_rng(11).standard_normal(A0.shape[0])
        x0 = np.zeros_like(b)
        S.solve_(x0, ns, b)
        assert lib.gmg_set_galerkin(h, 0) == abi.ERR_INVALID and b"level 0" in lib.gmg_last_error(h)
        assert lib.gmg_set_galerkin(h, 3) == abi.ERR_INVALID and lib.gmg_set_galerkin(h, -1) == abi.ERR_INVALID
        v = twin[1].val.copy()
        assert lib.gmg_update_values(h, 1, _p(v)) == abi.ERR_STATE and b"level 1" in lib.gmg_last_error(h)
        cp, ri = np.zeros(twin[1].shape[0] + 1, dtype=np.int64), np.zeros(v.size, dtype=np.int64)
        assert lib.gmg_update_values_csc(h, 1, _p(cp), _p(ri), _p(v), 0, 8) == abi.ERR_STATE and b"level 1" in lib.gmg_last_error(h)
        n, nnz = C.c_int64(), C.c_int64()
        assert lib.gmg_get_galerkin_matrix(h, 2, C.byref(n), C.byref(nnz), None, None, None, 0) == abi.ERR_STATE
        assert b"level 2" in lib.gmg_last_error(h)
        assert lib.gmg_get_galerkin_matrix(h, 0, C.byref(n), C.byref(nnz), None, None, None, 0) == abi.ERR_STATE
        assert lib.gmg_get_galerkin_matrix(h, 1, C.byref(n), C.byref(nnz), None, None, None, 0) == abi.OK      # the size query
        assert (n.value, nnz.value) == (twin[1].shape[0], twin[1].val.size)
        val = np.zeros(nnz.value)
        assert lib.gmg_get_galerkin_matrix(h, 1, None, None, None, None, _p(val), nnz.value - 1) == abi.ERR_INVALID
        assert lib.gmg_get_galerkin_matrix(h, 1, None, None, None, None, _p(val), nnz.value) == abi.OK
        assert np.array_equal(val, twin[1].val)
        x1 = np.zeros_like(b)
        S.solve_(x1, ns, b)
        assert np.array_equal(x0, x1)
    finally:
        ns.close()


def test_set_matrix_clears_the_mark_and_back(S, po, pkg):
    abi = pkg.abi
    A0, Ps, Rs, twin = _problem("q1_8x3")
    ns = _galerkin_ns(S, A0, Ps, Rs)
    lib, h = ns._lib, ns.h
    try:
        M = twin[1]
        p32 = M.ptr.astype(np.int32)
        abi.check(h, lib.gmg_set_matrix(h, 1, M.shape[0], M.shape[1], M.val.size, _p(p32), _p(M.idx), _p(M.val), abi.CSR, 0, 4))
        ns.setup()
        with pytest.raises(abi.GmgError) as e:
            ns.level_matrix(1)
        assert e.value.code == abi.ERR_STATE
        _equal(ns, 2, twin[2])                                # level 2 is still formed, from the matrix given for level 1
        abi.check(h, lib.gmg_set_galerkin(h, 1))             # and back: the matrix set on the level is dropped
        ns.setup()
        _equal(ns, 1, twin[1])
        _equal(ns, 2, twin[2])
    finally:
        ns.close()


def test_refused_at_setup(S, po, pkg):
    """a streamed matrix or transfer of the finer level and a communicator of two ranks: GMG_ERR_UNSUPPORTED naming the level; a
    missing prolongation: GMG_ERR_STATE.  Where the cause can be withdrawn the handle is set up again and solves as before (a
    communicator cannot be taken off a handle)."""
    abi = pkg.abi
    A0, Ps, Rs, twin = _problem("q1_8x3")
    b = np.random.default_rng(11).standard_normal(A0.shape[0])
    ns = _galerkin_ns(S, A0, Ps, Rs)
    lib, h = ns._lib, ns.h
    try:
        x0 = np.zeros_like(b)
        S.solve_(x0, ns, b)
        for op, M in ((abi.OP_A, A0), (abi.OP_P, Ps[0])):
            ptr, idx = M.ptr.astype(np.int64), M.idx.astype(np.int64)
            abi.check(h, lib.gmg_set_operator_rows(h, 0, op, M.shape[0], M.shape[1], 0, M.shape[0], _p(ptr), _p(idx), _p(M.val), 0, 8))
            with pytest.raises(abi.GmgError) as e:
                ns.setup()
            assert e.value.code == abi.ERR_UNSUPPORTED and "level 1" in str(e.value) and "streamed" in str(e.value)
            S._set_op(lib.gmg_set_matrix if op == abi.OP_A else lib.gmg_set_prolongation, h, 0, M)     # whole again
            ns.setup()
            _equal(ns, 1, twin[1])
            x1 = np.zeros_like(b)
            S.solve_(x1, ns, b)
            assert np.array_equal(x0, x1)
        xfn = abi.HOST_EXCHANGE_FN(lambda *a: None)
        rfn = abi.HOST_ALLREDUCE_FN(lambda *a: None)
        abi.check(h, lib.gmg_comm_init_host(h, 0, 1, C.cast(xfn, C.c_void_p), C.cast(rfn, C.c_void_p), None))
        abi.check(h, lib.gmg_comm_set_loopback(h, 2))
        with pytest.raises(abi.GmgError) as e:
            ns.setup()
        assert e.value.code == abi.ERR_UNSUPPORTED and "level 1" in str(e.value) and "communicator" in str(e.value)
    finally:
        ns.close()
    # a missing prolongation, on a handle built by hand
    h = C.c_void_p()
    abi.check(None, lib.gmg_create(C.byref(h), 2, 0))
    try:
        S._set_op(lib.gmg_set_matrix, h, 0, A0)
        abi.check(h, lib.gmg_set_galerkin(h, 1))
        abi.check(h, lib.gmg_set_smoother_jacobi(h, 0, abi.PRE_AND_POST, 10, 2.0 / 3.0))
        assert lib.gmg_setup(h) == abi.ERR_STATE and b"gmg_set_prolongation missing on level 0" in lib.gmg_last_error(h)
        S._set_op(lib.gmg_set_prolongation, h, 0, Ps[0])
        abi.check(h, lib.gmg_setup(h))
        n, nnz = C.c_int64(), C.c_int64()
        abi.check(h, lib.gmg_get_galerkin_matrix(h, 1, C.byref(n), C.byref(nnz), None, None, None, 0))
        val = np.zeros(nnz.value)
        abi.check(h, lib.gmg_get_galerkin_matrix(h, 1, None, None, None, None, _p(val), nnz.value))
        assert np.array_equal(val, gal.galerkin(None, A0, Ps[0])[1].val)                  # R = P^T
        x, res = np.zeros_like(b), abi.Result()
        abi.check(h, lib.gmg_apply(h, _p(b), _p(x), abi.MEM_HOST, C.byref(res), None, 0))
        assert np.all(np.isfinite(x)) and np.linalg.norm(x) > 0
    finally:
        lib.gmg_destroy(h)
