"""Plain references for the per-kernel checks of the full-size levels (no fixtures, no collection hooks).

The kernels the default options pick on the big levels (walk sweeps, the pair sweep in its eight-wave shape, the XCD remap, the
expanded "repeat" planes of a streamed operator, the 64-wide Gauss-Jordan coarse inverse) are selected by level size alone, so they
are checked on the levels the benchmark runs, at the rows where launch geometry goes wrong:

  edge_rows        the rows of a (nx, ny, nz)-node level where slices, planes, walk chains and the level itself begin and end
  row_reference    per sampled row: the float64 sum in CSR order, the exact value and the bound gamma_k * sum|a_ij x_j|
  check_rows       asserts a device result on sampled rows against row_reference (bit for bit unless the level sums with FMA taps)
  dot_reference    the exact dot and the bound of the order dot_partial_kernel + reduce_final_kernel sum in (either path)

"exact" = math.fsum of the error-free products (TwoProduct by Veltkamp splitting: a*b = p + e exactly), i.e. the exact sum
correctly rounded once."""
from __future__ import annotations

import itertools
import math

import numpy as np

U = 2.0 ** -53                      # unit roundoff of float64
ZWALK_T = 12                        # pat_zwalk_t: planes per chain of the walk kernels (include/gmg_amd.h)
K_BLOCK, RED_BLOCKS = 256, 1024     # kBlock, kRedBlocks of the two-stage dot (csrc/kernels.hpp)
RAGGED_NC, RAGGED_NLEV = (240, 232, 200), 4   # the ragged, anisotropic Q1 problem of tests/test_gpu_fullsize.py


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def two_product(a, b):
    """p = fl(a*b), e with a*b = p + e exactly (Dekker / Veltkamp; |a|, |b| far from overflow)."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    p = a * b
    sp = 134217729.0                # 2^27 + 1
    ca, cb = sp * a, sp * b
    ah = ca - (ca - a); al = a - ah
    bh = cb - (cb - b); bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


# ---------------------------------------------------------------- rows to sample
def edge_rows(nx, ny, nz, nrand=3000, seed=0, zwalk_t=ZWALK_T, per_plane=24):
    """Sorted unique rows of a level of nx * ny * nz nodes (x fastest): the first / last 130 rows; rows +-1 around every slice
    boundary of 64 and 128 rows in the first and the last plane; in the first, second, second-to-last and last z-plane and in every
    plane at a multiple of zwalk_t and its neighbours (every chain start / end, the ragged last chain included) the plane's first
    and last two rows, the ends of its first and last grid line, and `per_plane` seeded rows; `nrand` seeded rows anywhere."""
    P = nx * ny
    n = P * nz
    rng = np.random.default_rng(seed)
    parts = [np.arange(min(130, n)), np.arange(max(0, n - 130), n)]
    for plane in (0, nz - 1):
        for w in (64, 128):
            b = np.arange(0, P + w, w)
            parts.append(plane * P + (b[:, None] + np.array([-1, 0, 1])[None, :]).ravel().clip(0, P - 1))
    planes = {0, 1, nz - 2, nz - 1}
    for z in range(0, nz, zwalk_t):
        planes.update((z - 1, z, z + 1))
    planes.add(nz - 1 - (nz - 1) % zwalk_t)             # first plane of the last (ragged) chain
    local = np.array([0, 1, nx - 2, nx - 1, P - nx, P - nx + 1, P - 2, P - 1])
    for z in sorted(p for p in planes if 0 <= p < nz):
        parts.append(z * P + local.clip(0, P - 1))
        parts.append(z * P + rng.integers(0, P, per_plane))
    parts.append(rng.integers(0, n, nrand))
    return np.unique(np.concatenate(parts).astype(np.int64))


# ---------------------------------------------------------------- exact row reference
def padded_rows(ptr, idx, val, rows):
    """(cols[nr, k], vals[nr, k], lengths[nr]) of CSR rows `rows`, padded with column 0 / value 0.0."""
    rows = np.asarray(rows, dtype=np.int64)
    lo, hi = ptr[rows], ptr[rows + 1]
    ln = (hi - lo).astype(np.int64)
    k = int(ln.max()) if rows.size else 0
    j = np.arange(k)[None, :]
    m = j < ln[:, None]
    at = np.where(m, lo[:, None] + j, 0)
    cols = np.where(m, idx[at], 0).astype(np.int64)
    vals = np.where(m, val[at], 0.0)
    return cols, vals, ln


def row_reference(cols, vals, lengths, x):
    """For padded rows: (seq, exact, bound) -- seq the float64 sum taken left to right in CSR order from 0.0 (the reference's
    mul!), exact the exact row value rounded once, bound = gamma_k * sum_j |a_ij x_j| with k the stored row length: the largest
    error of ANY order of summing the rounded or FMA-fused products."""
    xs = np.asarray(x, dtype=np.float64)[cols]
    nr, k = cols.shape
    live = np.arange(k)[None, :] < lengths[:, None]
    seq = np.zeros(nr)
    for j in range(k):
        seq = np.where(live[:, j], seq + vals[:, j] * xs[:, j], seq)
    p, e = two_product(vals, xs)
    exact = np.array([math.fsum(itertools.chain(p[i, :lengths[i]].tolist(), e[i, :lengths[i]].tolist())) for i in range(nr)])
    bound = gamma(lengths) * np.sum(np.abs(vals * xs), axis=1)
    return seq, exact, bound


def fma_taps(sig):
    return "FM=1" in sig


def check_rows(y_rows, cols, vals, lengths, x, sig, what, bound_only=False, reference=None):
    """Device values of sampled rows against the row reference: bit for bit with the CSR-order sum when the level's kernels round
    products and sums separately (FM=0 in the signature), and within the bound in every case.  Returns the largest deviation from
    the exact value as a fraction of the bound (and in ulps of the exact value).
    bound_only: the bound alone (a layout that sums a row in another order, such as the lane tree of the CSR-stream kernel);
    reference: (seq, exact, bound) of these rows when the caller has them already."""
    seq, exact, bound = row_reference(cols, vals, lengths, x) if reference is None else reference
    y_rows = np.asarray(y_rows, dtype=np.float64)
    if not fma_taps(sig) and not bound_only:
        bad = np.nonzero(y_rows != seq)[0]
        assert bad.size == 0, f"{what} [{sig}]: {bad.size} of {y_rows.size} sampled rows differ from the CSR-order sum " \
                              f"(first at sample {bad[0]}: {y_rows[bad[0]]!r} vs {seq[bad[0]]!r})"
    dev = np.abs(y_rows - exact)
    assert np.all(dev <= bound), f"{what} [{sig}]: error beyond gamma_k * sum|a x| ({np.max(dev / np.maximum(bound, 1e-300)):.3g} of it)"
    frac = float(np.max(np.where(bound > 0, dev / np.maximum(bound, 1e-300), 0.0))) if dev.size else 0.0
    ulps = float(np.max(dev / np.maximum(np.spacing(np.abs(exact)), 5e-324))) if dev.size else 0.0
    return frac, ulps


def check_csr_rows(y, A, rows, x, sig, what):
    """check_rows for rows of a materialised CSR `A` (y = the whole device result)."""
    cols, vals, ln = padded_rows(A.ptr, A.idx, A.val, rows)
    return check_rows(np.asarray(y)[rows], cols, vals, ln, x, sig, what)


def check_stream_rows(y, M, planes, x, sig, what, per_plane=64, seed=0):
    """check_rows for a StreamedCSR: in every node plane of `planes` its first and last 130 rows and `per_plane` seeded rows, taken
    from M.plane_rows(z) (never the whole operator)."""
    rng = np.random.default_rng(seed)
    C, V, L, Y = [], [], [], []
    width = 0
    for z in planes:
        row0, B = M.plane_rows(int(z))
        nb = B.shape[0]
        loc = np.unique(np.concatenate([np.arange(min(130, nb)), np.arange(max(0, nb - 130), nb), rng.integers(0, nb, per_plane)]))
        c, v, ln = padded_rows(B.ptr, B.idx, B.val, loc)
        C.append(c); V.append(v); L.append(ln); Y.append(np.asarray(y)[row0 + loc])
        width = max(width, c.shape[1])
    pad = lambda a: np.pad(a, ((0, 0), (0, width - a.shape[1])))
    return check_rows(np.concatenate(Y), np.concatenate([pad(c) for c in C]), np.concatenate([pad(v) for v in V]),
                      np.concatenate(L), x, sig, what)


# ---------------------------------------------------------------- dot
def dot_exact(a, b, chunk=1 << 20):
    """sum a_i b_i, exact and rounded once (streamed through math.fsum chunk by chunk: no 2n-element list)."""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)

    def terms():
        for s in range(0, a.size, chunk):
            p, e = two_product(a[s:s + chunk], b[s:s + chunk])
            yield from p.tolist()
            yield from e.tolist()
    return math.fsum(terms())


def dot_depth(n, vec=True):
    """Longest chain of roundings a product passes through in dot_partial_kernel + reduce_final_kernel: the product itself,
    the lane's grid-stride accumulation (two terms per step of the 16-byte path, plus the odd tail on lane 0), the 64-lane
    butterfly (6), the four-wave combine (2), the strided accumulation of the <= 1024 partials over 256 lanes, again 6 + 2.
    It is NOT log2(n) + c: above nb * 256 * 2 elements the lanes accumulate sequentially (93 terms per lane at 288^3).
    vec = False: the path the kernel takes when an operand is not 16-byte aligned -- the same grid of nb workgroups, but one
    element per lane and step, ceil(n / (nb * 256)) terms per lane, and no odd tail."""
    n = int(n)
    nb = max(1, min(RED_BLOCKS, (n // 2 + K_BLOCK - 1) // K_BLOCK))
    if vec:
        lane = 2 * (-(-(n // 2) // (nb * K_BLOCK))) + (n & 1)
    else:
        lane = -(-n // (nb * K_BLOCK))
    return 1 + lane + 6 + 2 + (-(-nb // K_BLOCK)) + 6 + 2


def dot_reference(a, b, vec=True):
    """(exact, bound) with bound = gamma_{dot_depth(n, vec)} * sum |a_i b_i|."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return dot_exact(a, b), float(gamma(dot_depth(a.size, vec)) * np.sum(np.abs(a * b)))


def _tree(s, d):
    """block_sum of kernels.hpp on (..., 256) lanes: the xor butterfly over 64 lanes, then (sh0 + sh1) + (sh2 + sh3); s = values,
    d = chain lengths (-1: the lane holds the literal 0.0, adding it is exact) -> (value, chain) of thread 0"""
    def add(s1, d1, s2, d2):
        return s1 + s2, np.where((d1 >= 0) & (d2 >= 0), np.maximum(d1, d2) + 1, np.maximum(d1, d2))
    s = s.reshape(s.shape[:-1] + (4, 64)); d = d.reshape(s.shape)
    lane = np.arange(64)
    off = 32
    while off:
        s, d = add(s, d, s[..., lane ^ off], d[..., lane ^ off])
        off >>= 1
    s, d = s[..., 0], d[..., 0]
    s01, d01 = add(s[..., 0], d[..., 0], s[..., 1], d[..., 1])
    s23, d23 = add(s[..., 2], d[..., 2], s[..., 3], d[..., 3])
    return add(s01, d01, s23, d23)


def dot_emulate_scalar_path(a, b):
    """dot_partial_kernel with vec == 0 followed by reduce_final_kernel, operation by operation in float64 on the host:
    -> (value, length of the longest chain of roundings a product passed through)."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    n = a.size
    nb = max(1, min(RED_BLOCKS, (n // 2 + K_BLOCK - 1) // K_BLOCK))
    lanes = nb * K_BLOCK
    s, d = np.zeros(lanes), np.full(lanes, -1)
    for start in range(0, n, lanes):                       # one trip of the grid-stride loop: s += a[i] * b[i]
        m = min(lanes, n - start)
        s[:m] = s[:m] + a[start:start + m] * b[start:start + m]
        d[:m] = np.where(d[:m] >= 0, d[:m] + 1, 1)         # (0.0 + p is exact: the product's own rounding only)
    parts, dparts = _tree(s.reshape(nb, K_BLOCK), d.reshape(nb, K_BLOCK))
    s2, d2 = np.zeros(K_BLOCK), np.full(K_BLOCK, -1)
    for start in range(0, nb, K_BLOCK):                    # reduce_final_kernel: s += partials[i], i = lane, lane + 256, ...
        m = min(K_BLOCK, nb - start)
        s2[:m] = s2[:m] + parts[start:start + m]
        d2[:m] = np.where(d2[:m] >= 0, np.maximum(d2[:m], dparts[start:start + m]) + 1, dparts[start:start + m])
    v, c = _tree(s2, d2)
    return float(v), int(c)


# ---------------------------------------------------------------- per-kernel checks of every level of a Q1 hierarchy
TOL_KERNEL = 1e-13                  # per-kernel max|y - y_ref| / max|y_ref|


def max_rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def device_op(ns, lev, op, x, nout):
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.full((nout,), np.nan, dtype=torch.float64, device="cuda")   # (a row the kernel skips stays NaN)
    torch.cuda.synchronize()                        # the library runs on its own stream: torch's fill must be done first
    ns.op_apply(lev, op, xd, yd)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def check_q1_levels(ns, H, go, orc, families, seed=0, post_levels=(0,), coarse_tol=1e-12):
    """Every kernel of every level of a materialised Q1 hierarchy with the options ns was set up with, against the oracle `go`
    (orc.GMG of the same hierarchy and smoothers) and the exact row reference:
      op_apply OP_A / OP_R / OP_P on seeded inputs: the whole vector against orc.spmv bit for bit (rows summed in CSR order; bound
        only when the level's signature shows FMA taps), and the edge rows against the exact value within gamma_k * sum|a x|;
      smooth PRE on every level (POST too on `post_levels`) and precond against the oracle's at TOL_KERNEL;
      coarse_solve against go.coarse_solve (max_rel <= coarse_tol).
    `families` = {level: substring (or tuple of substrings) its sweep_signature must contain}: the kernel family the default picks at that size.  Every
    assertion message names the level's signature.  Returns one report line per level (signature, worst deviation from the exact
    value as a fraction of the bound and in ulps)."""
    from gridapsolvers_jl_amd import abi
    rng = np.random.default_rng(seed)
    nlev = len(H["mats"])
    report = []
    for l in range(nlev - 1):
        A = H["mats"][l]
        n = A.shape[0]
        x0, r0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
        x, r = x0.copy(), r0.copy()
        ns.smooth(l, x, r)                                  # (first: the signature is noted by the level's first sweep launch)
        sig = ns.sweep_signature(l)
        tag = f"level {l} ({n} rows) [{sig}]"
        if l in families:
            want = (families[l],) if isinstance(families[l], str) else families[l]
            assert all(w in sig for w in want), f"{tag}: the default for this size is {' '.join(want)}"
        xo, ro = go.smooth(l, x0, r0)
        assert max_rel(x, xo) <= TOL_KERNEL and max_rel(r, ro) <= TOL_KERNEL, (tag, "smooth PRE", max_rel(x, xo), max_rel(r, ro))
        if l in post_levels:
            x, r = x0.copy(), r0.copy()
            ns.smooth(l, x, r, which=abi.POST)
            xo, ro = go.smooth(l, x0, r0, post=True)
            assert max_rel(x, xo) <= TOL_KERNEL and max_rel(r, ro) <= TOL_KERNEL, (tag, "smooth POST", max_rel(x, xo), max_rel(r, ro))
        dx = np.zeros(n)
        ns.precond(l, r0, dx)
        assert max_rel(dx, go.precond(l, r0)) <= TOL_KERNEL, (tag, "precond", max_rel(dx, go.precond(l, r0)))
        nodes = tuple(c - 1 for c in H["ncells"][l])
        cnodes = tuple(c - 1 for c in H["ncells"][l + 1])
        fracs = []
        P, R = H["prolongations"][l], H["restrictions"][l]
        xc = rng.uniform(-1, 1, P.shape[1])
        for op, M, v, sample, name in ((abi.OP_A, A, x0, nodes, "OP_A"), (abi.OP_P, P, xc, nodes, "OP_P"), (abi.OP_R, R, x0, cnodes, "OP_R")):
            y = device_op(ns, l, op, v, M.shape[0])
            if not fma_taps(sig):
                ys = orc.spmv(M, v)
                nd = int(np.count_nonzero(y != ys))
                assert nd == 0, f"{tag} {name}: {nd} of {y.size} rows differ from the oracle's CSR-order mul! (max_rel {max_rel(y, ys):.3g})"
            fracs.append(check_csr_rows(y, M, edge_rows(*sample, seed=seed + l), v, sig, f"{tag} {name}"))
        report.append(f"level {l}: {n} rows  {sig}  |y - exact| <= {max(f[0] for f in fracs):.3g} of the bound ({max(f[1] for f in fracs):.2f} ulp)")
    A = H["mats"][-1]
    nL = A.shape[0]
    rc = rng.uniform(-1, 1, nL)
    y = device_op(ns, nlev - 1, abi.OP_A, rc, nL)
    assert np.array_equal(y, orc.spmv(A, rc)), f"coarsest level ({nL} rows) OP_A"
    xc = np.zeros(nL)
    ns.coarse_solve(rc, xc)
    dev = max_rel(xc, go.coarse_solve(rc))
    assert dev <= coarse_tol, f"coarsest level ({nL} dofs) coarse_solve: max_rel {dev:.3g} vs the oracle's pivoted LU"
    report.append(f"level {nlev - 1}: {nL} dofs  coarse_solve max_rel vs LU {dev:.3g}")
    return report


def check_dot(ns, n, seed, what="", offset=0):
    """ns.dot of two device vectors of length n against the exact dot: a random pair, and b = -a + tiny (heavy cancellation: the
    result is ~1e-12 of sum|a b|, so the bound, not a relative error, is the gate).  Returns the worst |d - exact| / bound.
    offset = k or (ka, kb): a and / or b are the views buf[k : k + n] of (n + k + 1)-element device tensors -- an odd k puts the
    vector 8 bytes off a 16-byte boundary, which takes dot_partial_kernel's one-element path; the bound is that path's."""
    import torch
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, n)
    out = 0.0
    ka, kb = (offset, offset) if np.isscalar(offset) else offset

    def place(v, k):
        if k == 0:
            return torch.from_numpy(v).cuda()
        buf = torch.zeros(n + k + 1, dtype=torch.float64, device="cuda")
        buf[k:k + n].copy_(torch.from_numpy(v))
        return buf[k:k + n]

    for b in (rng.uniform(-1, 1, n), -a + 1e-12 * rng.uniform(-1, 1, n)):
        ad, bd = place(a, ka), place(b, kb)
        vec = ad.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0
        assert vec == (ka % 2 == 0 and kb % 2 == 0), (ad.data_ptr() % 16, bd.data_ptr() % 16)
        torch.cuda.synchronize()
        d = ns.dot(ad, bd)
        ex, bound = dot_reference(a, b, vec)
        assert abs(d - ex) <= bound, f"dot n={n} offsets ({ka}, {kb}) {what}: {d!r} vs exact {ex!r}, bound {bound:.3g}"
        if not vec:                                        # the order is fixed and no product is contracted: the emulation's bits
            em = dot_emulate_scalar_path(a, b)[0]
            assert d == em, f"dot n={n} offsets ({ka}, {kb}) {what}: {d!r} is not the one-element path's sum {em!r}"
        out = max(out, abs(d - ex) / bound if bound > 0 else 0.0)
    return out


# ---------------------------------------------------------------- additive patch operator on sampled dofs of a streamed level
def patch_precond_reference(M, pp, pd, dofs, r):
    """(sum_p R_p^T A_p^{-1} R_p r)[dofs] -- one application of the additive patch operator (PatchSolvers.jl, omega = 1) at the
    sampled dofs -- with every block A_p = A[pd_p, pd_p] read from the rows M.plane_rows gives (one plane generated at a time) and
    solved by numpy's LU.  Only the patches that contain a sampled dof are formed."""
    pp = np.asarray(pp); pd = np.asarray(pd)
    n = M.shape[0]
    dofs = np.unique(np.asarray(dofs, dtype=np.int64))
    want = np.zeros(n, dtype=bool)
    want[dofs] = True
    hit = np.nonzero(want[pd])[0]
    patches = np.unique(np.searchsorted(pp, hit, side="right") - 1)
    plist = [pd[pp[p]:pp[p + 1]].astype(np.int64) for p in patches]
    rows = np.unique(np.concatenate(plist))
    _, B0 = M.plane_rows(0)
    per = B0.shape[0]
    del B0
    rowdata = {}
    for z in np.unique(rows // per):
        row0, B = M.plane_rows(int(z))
        for g in rows[(rows // per) == z]:
            i = int(g - row0)
            rowdata[int(g)] = (B.idx[B.ptr[i]:B.ptr[i + 1]].astype(np.int64), B.val[B.ptr[i]:B.ptr[i + 1]])
        del B
    w = max(len(d) for d in plist)
    Ab = np.tile(np.eye(w), (len(plist), 1, 1))
    rb = np.zeros((len(plist), w))
    for k, d in enumerate(plist):
        for a, g in enumerate(d):
            cols, vals = rowdata[int(g)]
            at = np.searchsorted(cols, d)
            ok = (at < cols.size) & (cols[np.minimum(at, cols.size - 1)] == d)
            Ab[k, a, :len(d)] = np.where(ok, vals[np.minimum(at, cols.size - 1)], 0.0)
        rb[k, :len(d)] = r[d]
    xb = np.linalg.solve(Ab, rb[:, :, None])[:, :, 0]
    out = np.zeros(n)
    for k, d in enumerate(plist):
        m = want[d]
        np.add.at(out, d[m], xb[k, :len(d)][m])
    return dofs, out[dofs]
