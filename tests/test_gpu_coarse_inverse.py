"""The dense coarse inverse (gmg_solver::build_dense_inverse: host BandLU, device Gauss-Jordan with 32- and 64-wide panels, then
dense_gemv_kernel per solve) on the nonsymmetric, edge-size, pivoting and singular families of tests/coarse_inverse_problems.py,
against numpy.linalg.solve refined in np.longdouble.  Every case is one two-level setup whose coarse matrix is the family's, and
coarse_solve(); the path is chosen with options= and confirmed with coarse_info().  tests/test_coarse_inverse_problems.py shows on
the host that a float64 restatement of the algorithm is a factor ten inside the gate used here and that wrong kernels are not.

1. 32-wide panels, matrix-core and scalar trailing update   2. 64-wide panels   3. the GEMV behind a host-built inverse
4. the whole inverse from unit vectors, and not its transpose   5. rejection by the device and fallback to the host LU
6. the host LU where it has to pivot; singular matrices   7. value refresh
(no block-solver case: the options of a block's engine cannot be set through the block API, so its LUSolver() blocks of this size
always take the host LU, which 6. covers)"""
import functools

import numpy as np
import pytest

import coarse_inverse_problems as ci
import fullsize_reference as fr

pytestmark = pytest.mark.gpu

GATE = fr.TOL_KERNEL
NEVER = 1.0e9                                                 # a gj_wide_min / coarse_host_max no family reaches
PATHS = {                                                     # options -> what coarse_info() has to say
    "mfma32": (dict(coarse_host_max=0, gj_wide_min=NEVER, gj_mfma=1), dict(built_by="device_gj", panel=32, mfma=True, device_rejected=False)),
    "scalar32": (dict(coarse_host_max=0, gj_wide_min=NEVER, gj_mfma=0), dict(built_by="device_gj", panel=32, mfma=False, device_rejected=False)),
    "wide64": (dict(coarse_host_max=0, gj_wide_min=1), dict(built_by="device_gj", panel=64, mfma=True, device_rejected=False)),
    "host": (dict(coarse_host_max=NEVER), dict(built_by="host_lu", panel=0, mfma=False, device_rejected=False)),
    "default": (dict(), None),
}
HOST_INFO = PATHS["host"][1]
FELL_BACK = dict(HOST_INFO, device_rejected=True)
PLAIN_SELL = dict(pattern=0, vdict=0, idx16=0, opattern=0)   # a layout that stores explicit values: gmg_setup refreshes in place


def _csr(po, M):
    return po.CSR(M.shape, M.indptr, M.indices, M.data)      # raw: duplicates stay two entries


def _setup(S, po, name, options, scale=1.0):
    c = ci.case(name)
    sm = S.RichardsonSmoother(S.JacobiLinearSolver(), 1, 1.0)
    gmg = S.GMGLinearSolver([_csr(po, c.A * scale), _csr(po, c.Ac * scale)], [_csr(po, c.P)], [_csr(po, c.R)], pre_smoothers=[sm],
                            post_smoothers=[sm], maxiter=1, mode="preconditioner", options=options)
    A = gmg.smatrices[0]
    return S.numerical_setup(S.symbolic_setup(gmg, A), A)


def _solve(ns, r):
    x = np.full(r.size, np.nan)
    ns.coarse_solve(r, x)
    return x


@functools.lru_cache(maxsize=None)
def _fresh(S, po, name, path, scale=1.0):
    """one fresh setup on the given path -> (x = coarse_solve(r), coarse_info(), device_bytes()); read-only"""
    options, want = PATHS[path]
    ns = _setup(S, po, name, options, scale)
    try:
        x = _solve(ns, ci.case(name).r)
        info, nbytes = ns.coarse_info(), ns.device_bytes()
    finally:
        ns.close()
    assert want is None or info == want, (name, path, info)
    x.setflags(write=False)
    return x, info, nbytes


def _check(S, po, name, path, tag):
    x = _fresh(S, po, name, path)[0]
    e = ci.max_rel(x, ci.reference(name))
    print("%s %s %s: %.3e" % (tag, name, path, e))
    assert e <= GATE, (name, path, e)
    return x


# ---------------------------------------------------------------- 1. 32-wide panels
@pytest.mark.parametrize("path", ["mfma32", "scalar32"])
@pytest.mark.parametrize("name", ["banded-%d" % n for n in ci.SIZES_32] + list(ci.DENSE) + ["duplicates-129"])
def test_narrow_panels_on_nonsymmetric_matrices(S, po, name, path):
    x = _check(S, po, name, path, "[32-wide]")
    ns = _setup(S, po, name, PATHS[path][0])                 # a second fresh setup: the same bits
    try:
        assert np.array_equal(_solve(ns, ci.case(name).r), x) and ns.coarse_info() == PATHS[path][1]
    finally:
        ns.close()
    if name == "duplicates-129":                             # two entries of one column add up to the value exactly: banded-129's bits
        assert np.array_equal(x, _fresh(S, po, "banded-129", path)[0])


# ---------------------------------------------------------------- 2. 64-wide panels
@pytest.mark.parametrize("name", ["banded-%d" % n for n in ci.SIZES_64] + ["dense-129"])
def test_wide_panels_on_nonsymmetric_matrices(S, po, name):
    x = _check(S, po, name, "wide64", "[64-wide]")
    d = ci.max_rel(x, _fresh(S, po, name, "mfma32")[0])
    print("[64-wide against 32-wide] %s: %.3e" % (name, d))
    assert d <= GATE, (name, d)


# ---------------------------------------------------------------- 3. the GEMV alone
@pytest.mark.parametrize("n", ci.SIZES_GEMV)
def test_gemv_behind_a_host_built_inverse(S, po, n):
    _check(S, po, "banded-%d" % n, "host", "[gemv]")


# ---------------------------------------------------------------- 4. the whole inverse
@pytest.mark.parametrize("path", ["mfma32", "scalar32", "wide64"])
@pytest.mark.parametrize("n", [65, 129])
def test_unit_vectors_reassemble_the_inverse_and_not_its_transpose(S, po, n, path):
    name = "banded-%d" % n
    ref = ci.inverse_reference(name)
    ns = _setup(S, po, name, PATHS[path][0])
    try:
        assert ns.coarse_info() == PATHS[path][1]
        Ainv = np.stack([_solve(ns, e) for e in np.eye(n)], axis=1)
    finally:
        ns.close()
    e, et = ci.max_rel(Ainv, ref), ci.max_rel(Ainv.T, ref)
    print("[inverse] %s %s: %.3e (transposed: %.3e)" % (name, path, e, et))
    assert e <= GATE and et > 1e3 * GATE, (name, path, e, et)


# ---------------------------------------------------------------- 5. rejection and fallback
REJECTED = [("pivot-97-first", "mfma32"), ("pivot-97-first", "scalar32"), ("pivot-97-first", "wide64"), ("pivot-97-last", "mfma32"),
            ("pivot-97-last", "wide64"), ("pivot-97-tiny", "mfma32"), ("pivot-97-tiny", "wide64"), ("pivot-1600-first", "default"),
            ("pivot-1600-last", "default")]


@pytest.mark.parametrize("name,path", REJECTED)
def test_device_rejects_what_needs_pivoting_and_the_host_takes_over(S, po, name, path):
    ns = _setup(S, po, name, PATHS[path][0])
    try:
        assert ns.coarse_info() == FELL_BACK, (name, path, ns.coarse_info())
        e = ci.max_rel(_solve(ns, ci.case(name).r), ci.reference(name))
        nbytes = ns.device_bytes()
    finally:
        ns.close()
    print("[fallback] %s %s: %.3e" % (name, path, e))
    assert e <= GATE, (name, path, e)
    # the scratch of the rejected inversion is gone: the footprint of a setup that chose the host LU at once
    assert nbytes == _fresh(S, po, name, "host")[2]


@pytest.mark.parametrize("name,path", REJECTED)
def test_without_a_fallback_the_rejection_is_an_error(S, po, pkg, name, path):
    with pytest.raises(pkg.abi.GmgError) as err:
        _setup(S, po, name, dict(PATHS[path][0], coarse_host_fallback_max=0))    # (the failed constructor destroys its handle)
    assert err.value.code == pkg.abi.ERR_SINGULAR and "pivoting" in str(err.value)
    assert ("zero pivot" in str(err.value)) == (not name.endswith("tiny")), str(err.value)


@pytest.mark.parametrize("path", ["mfma32", "wide64"])
def test_a_handle_survives_a_rejected_setup(S, po, pkg, path):
    """one handle: banded-97 on the device, then pivot-97-first (refused, no fallback), then banded-97 again"""
    good, bad = ci.case("banded-97"), ci.case("pivot-97-first")
    ns = _setup(S, po, "banded-97", dict(PATHS[path][0], coarse_host_fallback_max=0))
    try:
        x0 = _solve(ns, good.r)
        S._set_op(ns._lib.gmg_set_matrix, ns.h, 1, _csr(po, bad.Ac))
        with pytest.raises(pkg.abi.GmgError) as err:
            ns.setup()
        assert err.value.code == pkg.abi.ERR_SINGULAR and "zero pivot" in str(err.value)
        with pytest.raises(pkg.abi.GmgError) as err:
            _solve(ns, good.r)
        assert err.value.code == pkg.abi.ERR_STATE
        S._set_op(ns._lib.gmg_set_matrix, ns.h, 1, _csr(po, good.Ac))
        ns.setup()
        assert ns.coarse_info() == PATHS[path][1]
        assert np.array_equal(_solve(ns, good.r), x0)
        assert ns.device_bytes() == _fresh(S, po, "banded-97", path)[2]
    finally:
        ns.close()
    assert ci.max_rel(x0, ci.reference("banded-97")) <= GATE


# ---------------------------------------------------------------- 6. host LU with pivoting; singular matrices
@pytest.mark.parametrize("name", ci.BANDLU)
def test_host_lu_pivots_inside_an_unequal_band(S, po, name):
    x, info, _ = _fresh(S, po, name, "default")
    e = ci.max_rel(x, ci.reference(name))
    print("[host lu] %s: %.3e" % (name, e))
    assert info == HOST_INFO and e <= GATE, (name, info, e)


@pytest.mark.parametrize("path,says", [("default", "is singular"), ("mfma32", "pivoting"), ("scalar32", "pivoting"), ("wide64", "pivoting")])
def test_singular_matrix_is_refused_on_every_path(S, po, pkg, path, says):
    with pytest.raises(pkg.abi.GmgError) as err:
        _setup(S, po, "singular-65", dict(PATHS[path][0], coarse_host_fallback_max=0))
    assert err.value.code == pkg.abi.ERR_SINGULAR and says in str(err.value), str(err.value)
    if path != "default":                                     # with the fallback the host LU has the last word: singular
        with pytest.raises(pkg.abi.GmgError) as err:
            _setup(S, po, "singular-65", PATHS[path][0])
        assert err.value.code == pkg.abi.ERR_SINGULAR and "is singular" in str(err.value), str(err.value)


# ---------------------------------------------------------------- 7. value refresh
@pytest.mark.parametrize("path", ["mfma32", "wide64"])
def test_refreshed_values_give_the_bits_of_a_fresh_setup(S, po, path):
    name, scale = "banded-129", 1.7
    c = ci.case(name)
    options = dict(PATHS[path][0], **PLAIN_SELL)
    ns = _setup(S, po, name, options)
    try:
        info = ns.coarse_info()
        x1 = _solve(ns, c.r)
        S.numerical_setup_(ns, _csr(po, c.A * scale), smatrices=[_csr(po, c.A * scale), _csr(po, c.Ac * scale)])
        assert ns.coarse_info() == info == PATHS[path][1]
        x = _solve(ns, c.r)
    finally:
        ns.close()
    fresh = _setup(S, po, name, options, scale)
    try:
        assert np.array_equal(x, _solve(fresh, c.r))
    finally:
        fresh.close()
    assert not np.array_equal(x, x1)
    e = ci.max_rel(x, ci.reference(name, scale))
    print("[refresh] %s %s: %.3e" % (name, path, e))
    assert e <= GATE, (path, e)
