"""Worker of the multi-process tests (launched once per rank by test_distributed_*.py).

mode "numpy": CPU-only emulation of the distributed CG+GMG on this rank's LOCAL operators
              (partition.py) with gloo halo exchanges / all-reduces -- validates the
              partition, the exchange plans and the distributed algorithm without a GPU.
mode "gpu"  : the real thing through libgmgamd with the host-staged transport (several
              ranks may share one GPU), or RCCL when every rank has its own GPU.
Rank 0 compares the gathered solution with the serial CPU oracle and writes a JSON verdict."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def numpy_distributed_cg(local, rank, world, dist, torch, b_own, maxiter, atol, rtol, niter=10, omega=2.0 / 3.0, patches=None):
    """patches: None (Richardson-Jacobi) or per level (patch_ptr, local dofs, list of inverse blocks) -> the distributed patch
    smoother of PatchSolvers.jl:227-258: consistent!(b), local solves on the OWNED patches, assemble!(x), consistent!(x)."""
    import scipy.sparse.linalg as spla
    levels = local["levels"]
    nlev = len(levels)
    # (levels a rank holds nothing of -- they live on a rank subset, local["sub"] -- are None)
    A = [L.A.to_scipy() if L is not None else None for L in levels]
    P = [L.P.to_scipy() if L is not None and L.P is not None else None for L in levels[:-1]]
    R = [L.R.to_scipy() if L is not None and L.R is not None else None for L in levels[:-1]]
    dinv = [None if levels[l] is None else 1.0 / A[l].diagonal() if levels[l].overlap else 1.0 / A[l].diagonal()[: levels[l].n_own]
            for l in range(nlev - 1)]   # own x own diagonal (overlapping layout: every local row)
    sub = local.get("sub")
    from gridapsolvers_jl_amd import partition as _pa
    hints = ([(False, False)] * nlev if os.environ.get("GMG_NO_OVERLAP_HINTS", "0") != "0" or "order" not in local
             else _pa.overlap_hints(local, niter, "jacobi" if patches is None else "patch"))
    stats = {"exchanges": 0}
    rep_from, rep_gid = local["rep_from"], local["rep_gid"]
    Gc = A[nlev - 1].tocsc()                    # coarsest level is always replicated (global matrix)

    def exchange(l, v):
        L = levels[l] if isinstance(l, int) else l           # (a LocalLevel: the separate Krylov operator of a finest overlapping level)
        if L.nbr_rank.size:
            stats["exchanges"] += 1
        if L.overlap:                                # one local numbering: scatter through rcv_idx
            ops, keep = [], []
            for k, q in enumerate(L.nbr_rank):
                r0, r1 = L.rcv_ptr[k], L.rcv_ptr[k + 1]
                if r1 > r0:
                    t = torch.zeros(int(r1 - r0), dtype=torch.float64); keep.append((t, r0, r1))
                    ops.append(dist.P2POp(dist.irecv, t, int(q)))
                sidx = L.snd_idx[L.snd_ptr[k]:L.snd_ptr[k + 1]]
                if sidx.size:
                    ops.append(dist.P2POp(dist.isend, torch.from_numpy(v[sidx].copy()), int(q)))
            if ops:
                for w in dist.batch_isend_irecv(ops):
                    w.wait()
            for t, r0, r1 in keep:
                v[L.rcv_idx[r0:r1]] = t.numpy()
            return
        ops, keep = [], []
        for k, q in enumerate(L.nbr_rank):
            r0, r1 = L.rcv_ptr[k], L.rcv_ptr[k + 1]
            if r1 > r0:
                t = torch.zeros(int(r1 - r0), dtype=torch.float64); keep.append((t, r0, r1))
                ops.append(dist.P2POp(dist.irecv, t, int(q)))
            s = L.snd_idx[L.snd_ptr[k]:L.snd_ptr[k + 1]]
            if s.size:
                ops.append(dist.P2POp(dist.isend, torch.from_numpy(v[s].copy()), int(q)))
        if ops:
            for w in dist.batch_isend_irecv(ops):
                w.wait()
        for t, r0, r1 in keep:
            v[L.n_own + r0: L.n_own + r1] = t.numpy()

    def redistribute(plan, src, dst):
        """entries of `src` to the ranks that hold them in another partition of the same level (redistribute!,
        GridTransferOperators.jl:447-532): local ids on both sides, ascending global id per neighbour"""
        stats["redistributions"] = stats.get("redistributions", 0) + 1
        dst[plan["self_dst"]] = src[plan["self_src"]]
        ops, keep = [], []
        for k, q in enumerate(plan["nbr_rank"]):
            r0, r1 = plan["rcv_ptr"][k], plan["rcv_ptr"][k + 1]
            if r1 > r0:
                t = torch.zeros(int(r1 - r0), dtype=torch.float64); keep.append((t, r0, r1))
                ops.append(dist.P2POp(dist.irecv, t, int(q)))
            sidx = plan["snd_idx"][plan["snd_ptr"][k]:plan["snd_ptr"][k + 1]]
            if sidx.size:
                ops.append(dist.P2POp(dist.isend, torch.from_numpy(src[sidx].copy()), int(q)))
        if ops:
            for w in dist.batch_isend_irecv(ops):
                w.wait()
        for t, r0, r1 in keep:
            dst[plan["rcv_idx"][r0:r1]] = t.numpy()

    def shadow(l):
        """a rank that holds nothing of levels sub_from .. rep_from-1 still takes part in the collectives below them: the all-reduce
        that assembles the replicated residual (with a zero contribution)"""
        if l + 1 == rep_from:
            full = torch.zeros(levels[l + 1].n_own, dtype=torch.float64)
            dist.all_reduce(full)
        elif l + 1 < rep_from:
            shadow(l + 1)

    def assemble(l, v):
        """ghost -> owner add (reverse of `exchange`)"""
        L = levels[l]
        ops, keep = [], []
        for k, q in enumerate(L.nbr_rank):
            s0, s1 = L.snd_ptr[k], L.snd_ptr[k + 1]
            if s1 > s0:
                t = torch.zeros(int(s1 - s0), dtype=torch.float64); keep.append((t, s0, s1))
                ops.append(dist.P2POp(dist.irecv, t, int(q)))
            r0, r1 = L.rcv_ptr[k], L.rcv_ptr[k + 1]
            if r1 > r0:
                ops.append(dist.P2POp(dist.isend, torch.from_numpy(v[L.n_own + r0: L.n_own + r1].copy()), int(q)))
        if ops:
            for w in dist.batch_isend_irecv(ops):
                w.wait()
        for t, s0, s1 in keep:                               # neighbour order: deterministic sums
            np.add.at(v, L.snd_idx[s0:s1], t.numpy())

    def gdot(a, c):
        t = torch.tensor([float(np.dot(a, c))], dtype=torch.float64)
        dist.all_reduce(t)
        return float(t.item())

    def vec(l):
        return np.zeros(levels[l].n_own + levels[l].n_ghost)

    def smooth(l, x, r):
        n = levels[l].n_own
        if levels[l].overlap:
            # blocks of `depth` sweeps between two exchanges: consistent!(r) on every ghost layer, then every local row is swept
            # (ghost layer j stays exact for depth - j sweeps, the owned rows throughout)
            k = max(1, min(levels[l].depth, niter))
            for blk in range(0, niter, k):
                exchange(l, r)
                for _ in range(min(k, niter - blk)):
                    if patches is not None:
                        # additive Schwarz over EVERY vertex star inside the extended box: no assemble!, no exchange of dx
                        pp, pl, Binv = patches[l]
                        dx = np.zeros_like(r)
                        for p in range(pp.size - 1):
                            idx = pl[pp[p]:pp[p + 1]]
                            if idx.size:
                                dx[idx] += Binv[p] @ r[idx]
                        dx *= omega
                    else:
                        dx = omega * (dinv[l] * r)
                    x += dx
                    r -= A[l] @ dx
            return
        if patches is not None:
            pp, pl, Binv = patches[l]
            for _ in range(niter):
                exchange(l, r)                               # consistent!(b), PatchSolvers.jl:231
                dx = vec(l)
                for p in range(pp.size - 1):                 # owned patches, ascending (PatchSolvers.jl:288)
                    idx = pl[pp[p]:pp[p + 1]]
                    if idx.size:
                        dx[idx] += Binv[p] @ r[idx]
                assemble(l, dx)                              # PatchSolvers.jl:254
                dx[n:] = 0.0
                dx[:n] *= omega
                x[:n] += dx[:n]
                exchange(l, dx)                              # consistent!(x), :256
                r[:n] -= A[l] @ dx
            return
        for _ in range(niter):
            dx = vec(l)
            dx[:n] = omega * (dinv[l] * r[:n])
            x[:n] += dx[:n]
            exchange(l, dx)
            r[:n] -= A[l] @ dx

    def cycle(l, x, r):
        n = levels[l].n_own
        if l == nlev - 1:
            x[:n] = spla.spsolve(Gc, r[:n])
            return
        smooth(l, x, r)
        if not (levels[l].overlap and hints[l][0]):
            exchange(l, r)                       # (skipped when the last smoothing block left the layers R reads exact)
        if sub is not None and l + 1 == sub["sub_from"]:
            # level l+1 lives on a rank subset: restrict in the glued partition, redistribute, recurse on the members, bring the
            # correction back to the glued own AND ghost entries (P reads both)
            rg = R[l] @ r
            rH, dxH = np.zeros(sub["n_sub_local"]), np.zeros(sub["n_sub_local"])
            redistribute(sub["to_sub"], rg, rH)
            if sub["member"]:
                cycle(l + 1, dxH, rH)
            else:
                shadow(l + 1)
            xg = np.zeros(sub["n_glue_own"] + sub["n_glue_ghost"])
            redistribute(sub["from_sub"], dxH, xg)
            if levels[l].overlap:
                dx = P[l] @ xg
                x += dx
                exchange(l, dx)
                r -= A[l] @ dx
            else:
                dx = vec(l); dx[:n] = P[l] @ xg
                x[:n] += dx[:n]
                exchange(l, dx)
                r[:n] -= A[l] @ dx
            smooth(l, x, r)
            return
        rH = vec(l + 1)
        if l + 1 == rep_from:                    # distributed -> replicated boundary: assemble by all-reduce
            full = torch.zeros(levels[l + 1].n_own, dtype=torch.float64)
            full[torch.from_numpy(rep_gid)] = torch.from_numpy(R[l] @ r)
            dist.all_reduce(full)
            rH[:] = full.numpy()
        elif levels[l + 1].overlap:
            rH[:] = R[l] @ r                     # rows of ghost coarse entries are empty
        else:
            rH[: levels[l + 1].n_own] = R[l] @ r
        dxH = vec(l + 1)
        cycle(l + 1, dxH, rH)
        exchange(l + 1, dxH)
        if levels[l].overlap:                    # every local row (ghost rows are fixed by the exchange below)
            dx = P[l] @ dxH
            x += dx
            if not hints[l][1]:
                exchange(l, dx)                  # (skipped when P's rows are complete wherever r_own -= (A dx)_own reads dx)
            r -= A[l] @ dx
        else:
            dx = vec(l); dx[:n] = P[l] @ dxH
            x[:n] += dx[:n]
            exchange(l, dx)
            r[:n] -= A[l] @ dx
        smooth(l, x, r)

    n = levels[0].n_own
    K = local.get("krylov")
    if K is not None:
        # finest level in the overlapping layout: the Krylov vectors stay own | ghost (operator K.A, one exchange per mat-vec), the
        # preconditioner works in level 0's extended-box numbering -- r scattered in, the owned entries of z gathered out
        AK = K.A.to_scipy()
        x, p, z, r = (np.zeros(K.n_own + K.n_ghost) for _ in range(4))
        r[:n] = b_own
        gamma = 1.0
        res = np.sqrt(gdot(r[:n], r[:n])); hist = [res]
        it = 0
        done = (it >= maxiter) or (1.0 < rtol) or (res < atol)
        while not done:
            ze, re = vec(0), vec(0)
            re[K.own_idx] = r[:n]
            cycle(0, ze, re)
            z[:n] = ze[K.own_idx]
            beta = gamma; gamma = gdot(z[:n], r[:n]); beta = gamma / beta
            p[:n] = z[:n] + beta * p[:n]
            exchange(K, p)
            w = AK @ p
            alpha = gamma / gdot(p[:n], w)
            x[:n] += alpha * p[:n]
            r[:n] -= alpha * w
            res = np.sqrt(gdot(r[:n], r[:n])); hist.append(res); it += 1
            done = (it >= maxiter) or (res / hist[0] < rtol) or (res < atol)
        numpy_distributed_cg.last_exchanges = stats["exchanges"]
        numpy_distributed_cg.last_redistributions = stats.get("redistributions", 0)
        return x[:n].copy(), it, np.array(hist)
    x, p, z = vec(0), vec(0), vec(0)
    r = vec(0); r[:n] = b_own                      # x0 = 0
    gamma = 1.0
    res = np.sqrt(gdot(r[:n], r[:n])); hist = [res]
    it = 0
    done = (it >= maxiter) or (1.0 < rtol) or (res < atol)
    while not done:
        z[:] = 0.0
        rr = r.copy()
        cycle(0, z, rr)
        beta = gamma; gamma = gdot(z[:n], r[:n]); beta = gamma / beta
        p[:n] = z[:n] + beta * p[:n]
        exchange(0, p)
        w = A[0] @ p
        alpha = gamma / gdot(p[:n], w)
        x[:n] += alpha * p[:n]
        r[:n] -= alpha * w
        res = np.sqrt(gdot(r[:n], r[:n])); hist.append(res); it += 1
        done = (it >= maxiter) or (res / hist[0] < rtol) or (res < atol)
    numpy_distributed_cg.last_exchanges = stats["exchanges"]
    numpy_distributed_cg.last_redistributions = stats.get("redistributions", 0)
    return x[:n].copy(), it, np.array(hist)


def block_mode(cells, nlev, out, transport, rank, world, dist, torch, pkg, po, pa, multigpu, grid, cg):
    """Distributed block-triangular preconditioner + FGMRES on a saddle point built from two levels of the partitioned
    hierarchy (blocks: A_0, c R_0^T; c R_0, -(1/alpha)(I + 0.1 A_1)), GMG(maxiter=4) on block 0, CG-Jacobi on block 1 --
    the solver shape of test/Applications/mpi/StokesGMG.jl -- against the serial oracle."""
    import scipy.sparse as sp
    alpha, cb = 10.0, 0.05
    ndev = torch.cuda.device_count()
    dev = rank % max(ndev, 1)
    torch.cuda.set_device(dev)
    g = multigpu.DistributedGMG(cells, nlev, rank, world, device_id=dev, transport=transport, group=None, rep_from=2,
                                gmg_maxiter=4, gmg_rtol=1e-8)
    L0, L1 = g.local["levels"][0], g.local["levels"][1]

    def scaled(M, c):
        return po.CSR(M.shape, M.ptr, M.idx, c * M.val)
    A01 = scaled(L0.P, cb)                               # c P_0 = (c R_0)^T, rows: own fine, cols: [own | ghost] coarse
    A10 = scaled(L0.R, cb)
    n2 = L1.n_own
    I_loc = sp.csr_matrix((np.ones(n2), (np.arange(n2), np.arange(n2))), shape=(n2, n2 + L1.n_ghost))
    Mloc = ((-1.0 / alpha) * (I_loc + 0.1 * L1.A.to_scipy())).tocsr(); Mloc.sort_indices()
    M11 = po.CSR(Mloc.shape, Mloc.indptr, Mloc.indices, Mloc.data)
    blk = multigpu.DistributedBlockSolver(g, A01, A10, M11, L0, L1, A11=M11)
    N1, N2 = po.level_sizes(cg, 1), po.level_sizes(tuple(c // 2 for c in cg), 1)
    bg = np.random.default_rng(5).uniform(-1, 1, N1 + N2)
    b = np.concatenate([bg[:N1][L0.own_gid], bg[N1:][L1.own_gid]])
    z = np.zeros_like(b)
    blk.precond_apply(b, z)
    x = np.zeros_like(b)
    log = blk.fgmres_solve(b, x, m=20, maxiter=100, atol=1e-10, rtol=1e-12)
    parts = [None] * world
    dist.all_gather_object(parts, (L0.own_gid, L1.own_gid, x, z, int(log.num_iters), log.residuals[: log.num_iters + 1].tolist()))
    if rank == 0:
        orc = entry.import_oracle()
        H = po.build_hierarchy(cg, nlev, 1)
        A, R = H["mats"][0], H["restrictions"][0]
        B = po.CSR(R.shape, R.ptr, R.idx, cb * R.val)
        Bts = (cb * R.to_scipy().T).tocsr(); Bts.sort_indices()
        Bt = po.CSR(Bts.shape, Bts.indptr, Bts.indices, Bts.data)
        Mps = ((-1.0 / alpha) * (sp.identity(N2) + 0.1 * H["mats"][1].to_scipy())).tocsr(); Mps.sort_indices()
        Mp = po.CSR(Mps.shape, Mps.indptr, Mps.indices, Mps.data)
        Ks = sp.bmat([[A.to_scipy(), Bts], [B.to_scipy(), Mps]]).tocsr(); Ks.sort_indices()
        K = po.CSR(Ks.shape, Ks.indptr, Ks.indices, Ks.data)
        go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], maxiter=4, rtol=1e-8)
        Po = orc.BlockPreconditioner([N1, N2], [go, (orc.BD_CG_JACOBI, Mp, 20, 1e-14, 1e-6)], {(0, 1): (Bt, 1.0), (1, 0): (B, 0.0)}, orc.UPPER)
        zo = Po.apply(bg)
        go2 = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], maxiter=4, rtol=1e-8)
        Po2 = orc.BlockPreconditioner([N1, N2], [go2, (orc.BD_CG_JACOBI, Mp, 20, 1e-14, 1e-6)], {(0, 1): (Bt, 1.0), (1, 0): (B, 0.0)}, orc.UPPER)
        xo, nit, flag, hist = orc.fgmres_solve(K, bg, Pr=Po2, m=20, maxiter=100, atol=1e-10, rtol=1e-12)
        xg, zg = np.zeros(N1 + N2), np.zeros(N1 + N2)
        for g0, g1, xq, zq, _, _ in parts:
            xg[g0] = xq[: g0.size]; xg[N1 + g1] = xq[g0.size:]
            zg[g0] = zq[: g0.size]; zg[N1 + g1] = zq[g0.size:]
        hist_d = np.array(parts[0][5])
        verdict = dict(iters=int(parts[0][4]), iters_oracle=int(nit), iters_all_equal=all(p[4] == parts[0][4] for p in parts),
                       precond_rel_err=float(np.linalg.norm(zg - zo) / np.linalg.norm(zo)),
                       rel_err=float(np.linalg.norm(xg - xo) / np.linalg.norm(xo)),
                       hist_dev=float(np.max(np.abs(hist_d - hist) / hist[0])) if len(hist_d) == len(hist) else 1.0,
                       true_residual=float(np.linalg.norm(Ks @ xg - bg)), world=world, grid=list(grid), mode="gpu_block")
        json.dump(verdict, open(out, "w"))
    dist.barrier()
    blk.close(); g.close()
    dist.destroy_process_group()


def stokes_mode(n, nlev, out, transport, rank, world, dist, torch, pkg, po, pa, multigpu):
    """test/Applications/mpi/StokesGMG.jl:5-12 on the synthesised lid-driven cavity (stokes.py): vector-valued Q2 velocity and
    discontinuous P1 pressure partitioned by cell boxes (dpartition.py), distributed velocity GMG(maxiter=4) with owned
    vertex-star patch smoothers (caller-assembled patch matrices, assemble!) and the patch-corrected prolongation with the
    grad-div rhs form, CG-Jacobi pressure block, upper block-triangular preconditioner, FGMRES(20) -- against the serial oracle."""
    from gridapsolvers_jl_amd import stokes as st, dpartition as dp
    alpha = 1.0e3
    ndev = torch.cuda.device_count()
    dev = rank % max(ndev, 1)
    torch.cuda.set_device(dev)
    grid = pa.rank_grid(world, 2)
    sysd, Hv = st.stokes_system(n, alpha), st.velocity_hierarchy(n, nlev, alpha)
    cells, npart = Hv["ncells"], nlev - 1                        # levels 0 .. nlev-2 partitioned, the coarsest replicated
    V = [dp.Space(f"v{l}", st.velocity_owner(cells[l], grid), world) for l in range(nlev)]
    Pq = dp.Space("p", st.pressure_owner(n, grid), world)
    A = sysd["A"]
    sc = lambda M: M.to_scipy()
    ops = [(sc(A[0][0]), V[0], V[0]), (sc(A[0][1]), V[0], Pq), (sc(A[1][0]), Pq, V[0]), (sc(sysd["Mp_scaled"]), Pq, Pq)]
    pats, star_own, int_own = [], [], []
    for l in range(npart):
        ops += [(sc(Hv["mats"][l]), V[l], V[l]), (sc(Hv["graddiv"][l]), V[l], V[l]), (sc(Hv["restrictions"][l]), V[l + 1], V[l])]
        if l + 1 < npart:
            ops.append((sc(Hv["prolongations"][l]), V[l], V[l + 1]))
        star_own.append(st.patch_owner(*Hv["star_patches"][l], V[l].owner))
        int_own.append(st.patch_owner(*Hv["interior_patches"][l], V[l].owner))
        pats += [(*Hv["star_patches"][l], V[l], star_own[l]), (*Hv["interior_patches"][l], V[l], int_own[l])]
    dp.partition_spaces(V + [Pq], ops, pats)
    # GMG_TEST_DEPTH > 0: the partitioned velocity levels >= 1 in the OVERLAPPING layout (dpartition.OverlapSpace: node box + 4 * depth
    # node layers -- a sweep of Richardson(PatchSolver) on Q2 vertex stars consumes 3 * 2 - 2 = 4), both components of a node together
    depth = int(os.environ.get("GMG_TEST_DEPTH", "0"))

    def node_coords(c):
        k = np.arange((2 * c - 1) ** 2)
        xy = np.stack([k % (2 * c - 1) + 1, k // (2 * c - 1) + 1], axis=1)
        return np.repeat(xy, 2, axis=0)
    OV = {l: dp.OverlapSpace(f"ov{l}", V[l].owner, node_coords(cells[l]), world, 4 * depth) for l in range(1, npart)} if depth > 0 else {}

    class LL:
        overlap = False

    def plan_of(obj, S):
        pl = S.plan[rank]
        obj.n_own, obj.n_ghost = S.n_own(rank), S.n_ghost(rank)
        obj.nbr_rank, obj.snd_ptr, obj.snd_idx, obj.rcv_ptr = pl["nbr_rank"], pl["snd_ptr"], pl["snd_idx"], pl["rcv_ptr"]
    levels, ptabs, ctabs = [], [], []
    rep_gid = np.zeros(0, dtype=np.int64)
    for l in range(nlev):
        L = LL()
        if l in OV:
            S, pl = OV[l], OV[l].plan[rank]
            L.replicated, L.overlap, L.depth = False, True, depth
            L.n_local, L.n_own = S.n_local(rank), S.n_own(rank)
            L.n_ghost = L.n_local - L.n_own
            L.nbr_rank, L.snd_ptr, L.snd_idx, L.rcv_ptr, L.rcv_idx = pl["nbr_rank"], pl["snd_ptr"], pl["snd_idx"], pl["rcv_ptr"], pl["rcv_idx"]
            L.A = S.square(sc(Hv["mats"][l]), rank)
            if l + 1 in OV:
                Cs = OV[l + 1]
                L.P = dp.sliced_operator(sc(Hv["prolongations"][l]), S.ext[rank], Cs.g2l[rank], ncols=Cs.n_local(rank))
                L.R = dp.sliced_operator(sc(Hv["restrictions"][l]), Cs.ext[rank], S.g2l[rank], keep_row=Cs.is_own[rank], ncols=S.n_local(rank),
                                         strict_rows=Cs.is_own[rank])
            else:                                               # boundary to the replicated level
                L.P = dp.sliced_operator(sc(Hv["prolongations"][l]), S.ext[rank])
                rows = V[l + 1].own[rank]
                L.R = dp.sliced_operator(sc(Hv["restrictions"][l]), rows, S.g2l[rank], ncols=S.n_local(rank), strict_rows=np.ones(rows.size, bool))
                rep_gid = rows
            ptr, loc = S.patches(*Hv["star_patches"][l], rank)
            ptabs.append((ptr, loc, None))                      # blocks A[p,p] from the local matrix
            cptr, cloc = S.patches(*Hv["interior_patches"][l], rank)
            ctabs.append((cptr, cloc, S.square(sc(Hv["graddiv"][l]), rank)))
        elif l < npart:
            plan_of(L, V[l])
            L.replicated = False
            L.A = dp.local_operator(sc(Hv["mats"][l]), V[l], V[l], rank)
            if l + 1 in OV:                                     # own | ghost fine level, overlapping coarse level
                Cs = OV[l + 1]
                L.P = dp.sliced_operator(sc(Hv["prolongations"][l]), V[l].own[rank], Cs.g2l[rank], ncols=Cs.n_local(rank),
                                         strict_rows=np.ones(V[l].n_own(rank), bool))
                L.R = dp.sliced_operator(sc(Hv["restrictions"][l]), Cs.ext[rank], V[l].g2l[rank], keep_row=Cs.is_own[rank],
                                         ncols=V[l].n_own(rank) + V[l].n_ghost(rank), strict_rows=Cs.is_own[rank])
            elif l + 1 < npart:
                L.P = dp.local_operator(sc(Hv["prolongations"][l]), V[l], V[l + 1], rank)
                L.R = dp.local_operator(sc(Hv["restrictions"][l]), V[l + 1], V[l], rank)
            else:                                               # boundary to the replicated level: global coarse columns, this rank's coarse rows
                Pg = sc(Hv["prolongations"][l]).tocsr()[V[l].own[rank]]
                Pg.sort_indices()
                L.P = po.CSR(Pg.shape, Pg.indptr.astype(np.int64), Pg.indices.astype(np.int32), Pg.data)
                L.R = dp.local_operator(sc(Hv["restrictions"][l]), V[l + 1], V[l], rank)
                rep_gid = V[l + 1].own[rank]
            ptr, loc, _g, blocks = dp.local_patches(*Hv["star_patches"][l], V[l], star_own[l], rank, sc(Hv["mats"][l]))
            ptabs.append((ptr, loc, blocks))
            cptr, cloc, _cg, _ = dp.local_patches(*Hv["interior_patches"][l], V[l], int_own[l], rank)
            ctabs.append((cptr, cloc, dp.local_operator(sc(Hv["graddiv"][l]), V[l], V[l], rank)))
        else:
            L.replicated = True
            L.A = Hv["mats"][l]
            L.n_own, L.n_ghost = L.A.shape[0], 0
            ptabs.append(None); ctabs.append(None)
        levels.append(L)
    local = dict(levels=levels, rep_from=npart, rep_gid=np.ascontiguousarray(rep_gid, dtype=np.int64), cells=[(c, c) for c in cells],
                 grid=grid, order=2, rank=rank, nranks=world)
    g = multigpu.DistributedGMG((n // grid[0], n // grid[1]), nlev, rank, world, device_id=dev, transport=transport, order=2, niter=10, omega=0.2,
                                gmg_maxiter=4, gmg_rtol=1e-8, local_hierarchy=local, smoother="patch", patch_tables=ptabs, pcorr_tables=ctabs,
                                cells_global=(n, n))
    nu, npp = sysd["sizes"]
    # (1) the distributed velocity GMG alone
    rg = np.random.default_rng(2).uniform(-1, 1, nu)
    z = np.zeros(V[0].n_own(rank))
    ex0 = g.comm_stats()[0]
    glog = g.apply(np.ascontiguousarray(rg[V[0].own[rank]]), z, maxiter=4)
    # (2) the whole solve
    lev1 = LL(); plan_of(lev1, Pq)
    A01 = dp.local_operator(sc(A[0][1]), V[0], Pq, rank)
    A10 = dp.local_operator(sc(A[1][0]), Pq, V[0], rank)
    M11 = dp.local_operator(sc(sysd["Mp_scaled"]), Pq, Pq, rank)
    blk = multigpu.DistributedBlockSolver(g, A01, A10, M11, levels[0], lev1, A11=None, coeffs=((1.0, 1.0), (0.0, 1.0)), half="upper", cg=(20, 1e-14, 1e-6))
    bg = sysd["b"]
    b = np.concatenate([bg[:nu][V[0].own[rank]], bg[nu:][Pq.own[rank]]])
    x = np.zeros_like(b)
    log = blk.fgmres_solve(b, x, m=20, maxiter=100, atol=1e-10, rtol=1e-12)
    n_exchanges = int(g.comm_stats()[0] - ex0)
    parts = [None] * world
    dist.all_gather_object(parts, (V[0].own[rank], Pq.own[rank], x, z, int(log.num_iters), log.residuals[: log.num_iters + 1].tolist(), int(glog.num_iters)))
    if rank == 0:
        orc = entry.import_oracle()
        osm = [orc.Smoother(orc.PATCH, 10, 0.2, pp, pd) for pp, pd in Hv["star_patches"]]

        def make_go():
            return orc.GMG(Hv["mats"], Hv["prolongations"], Hv["restrictions"], pre_smoothers=osm, maxiter=4, rtol=1e-8,
                           prolongation_patches=[(orc.PATCH, *Hv["interior_patches"][l], Hv["graddiv"][l]) for l in range(nlev - 1)])
        zo, nit_g, _, _ = make_go().solve(rg)
        Po = orc.BlockPreconditioner([nu, npp], [make_go(), (orc.BD_CG_JACOBI, sysd["Mp_scaled"], 20, 1e-14, 1e-6)],
                                     {(0, 1): (A[0][1], 1.0), (1, 0): (A[1][0], 0.0)}, orc.UPPER)
        K = sysd["K"]
        Kc = po.CSR(K.shape, K.indptr, K.indices, K.data)
        xo, nit, flag, hist = orc.fgmres_solve(Kc, bg, Pr=Po, m=20, maxiter=100, atol=1e-10, rtol=1e-12)
        xg, zg = np.zeros(nu + npp), np.zeros(nu)
        for vo, pown, xq, zq, _, _, _ in parts:
            xg[vo] = xq[: vo.size]; xg[nu + pown] = xq[vo.size:]
            zg[vo] = zq
        hist_d = np.array(parts[0][5])
        verdict = dict(iters=int(parts[0][4]), iters_oracle=int(nit), iters_all_equal=all(p[4] == parts[0][4] for p in parts),
                       gmg_iters=int(parts[0][6]), gmg_iters_oracle=int(nit_g),
                       gmg_rel_err=float(np.linalg.norm(zg - zo) / np.linalg.norm(zo)),
                       rel_err=float(np.linalg.norm(xg - xo) / np.linalg.norm(xo)),
                       hist_dev=float(np.max(np.abs(hist_d - hist) / hist[0])) if len(hist_d) == len(hist) else 1.0,
                       true_residual=float(np.linalg.norm(K @ xg - bg)), div_residual=float(np.linalg.norm(sc(A[1][0]) @ xg[:nu] - bg[nu:])),
                       umax=float(xg[:nu].max()), world=world, grid=list(grid), mode="gpu_stokes", exchanges=n_exchanges,
                       overlap_levels=sorted(OV), local_entries=[int(OV[l].n_local(0)) for l in sorted(OV)],
                       ghosts=[int(V[0].n_ghost(0)), int(Pq.n_ghost(0))])
        json.dump(verdict, open(out, "w"))
    dist.barrier()
    blk.close(); g.close()
    dist.destroy_process_group()


def stokes_matvec_mode(n, nlev, out, rank, world, dist, torch, pkg, po, pa):
    """CPU / gloo: the partitioned Q2 / P1disc Stokes block system applied with real neighbour exchanges -- every rank holds its
    rows of the four blocks in [own | ghost] column numbering (dpartition.py), makes its ghosts consistent (consistent!) through
    the exchange plans and applies its rows; the gathered result must be K x.  Also the reverse halo (assemble!) on the velocity
    space: ghost contributions added to their owners reproduce a global scatter-add."""
    from gridapsolvers_jl_amd import stokes as st, dpartition as dp
    grid = pa.rank_grid(world, 2)
    sysd, Hv = st.stokes_system(n), st.velocity_hierarchy(n, nlev)
    V0 = dp.Space("v0", st.velocity_owner(n, grid), world)
    Pq = dp.Space("p", st.pressure_owner(n, grid), world)
    A = sysd["A"]
    sc = lambda M: M.to_scipy()
    ops = [(sc(A[0][0]), V0, V0), (sc(A[0][1]), V0, Pq), (sc(A[1][0]), Pq, V0)]
    pp, pd = Hv["star_patches"][0]
    dp.partition_spaces([V0, Pq], ops, [(pp, pd, V0, st.patch_owner(pp, pd, V0.owner))])

    def exchange(S, v):
        pl = S.plan[rank]
        reqs, keep = [], []
        for k, q in enumerate(pl["nbr_rank"]):
            r0, r1 = pl["rcv_ptr"][k], pl["rcv_ptr"][k + 1]
            if r1 > r0:
                t = torch.zeros(int(r1 - r0), dtype=torch.float64); keep.append((t, r0, r1))
                reqs.append(dist.P2POp(dist.irecv, t, int(q)))
            sidx = pl["snd_idx"][pl["snd_ptr"][k]:pl["snd_ptr"][k + 1]]
            if sidx.size:
                reqs.append(dist.P2POp(dist.isend, torch.from_numpy(v[sidx].copy()), int(q)))
        if reqs:
            for w in dist.batch_isend_irecv(reqs):
                w.wait()
        for t, r0, r1 in keep:
            v[S.n_own(rank) + r0: S.n_own(rank) + r1] = t.numpy()

    def assemble(S, v):
        pl = S.plan[rank]
        reqs, keep = [], []
        for k, q in enumerate(pl["nbr_rank"]):
            s0, s1 = pl["snd_ptr"][k], pl["snd_ptr"][k + 1]
            if s1 > s0:
                t = torch.zeros(int(s1 - s0), dtype=torch.float64); keep.append((t, s0, s1))
                reqs.append(dist.P2POp(dist.irecv, t, int(q)))
            r0, r1 = pl["rcv_ptr"][k], pl["rcv_ptr"][k + 1]
            if r1 > r0:
                reqs.append(dist.P2POp(dist.isend, torch.from_numpy(v[S.n_own(rank) + r0: S.n_own(rank) + r1].copy()), int(q)))
        if reqs:
            for w in dist.batch_isend_irecv(reqs):
                w.wait()
        for t, s0, s1 in keep:
            np.add.at(v, pl["snd_idx"][s0:s1], t.numpy())
    nu, npp = sysd["sizes"]
    xg = np.random.default_rng(4).uniform(-1, 1, nu + npp)
    xu = np.zeros(V0.n_own(rank) + V0.n_ghost(rank)); xu[: V0.n_own(rank)] = xg[:nu][V0.own[rank]]
    xp = np.zeros(Pq.n_own(rank) + Pq.n_ghost(rank)); xp[: Pq.n_own(rank)] = xg[nu:][Pq.own[rank]]
    exchange(V0, xu); exchange(Pq, xp)
    yu = dp.local_operator(sc(A[0][0]), V0, V0, rank).matvec(xu) + dp.local_operator(sc(A[0][1]), V0, Pq, rank).matvec(xp)
    yp = dp.local_operator(sc(A[1][0]), Pq, V0, rank).matvec(xu)
    # assemble!: every rank adds 1 + rank to all its local velocity entries; owners must end up with the sum over the ranks that see the dof
    w = np.full(V0.n_own(rank) + V0.n_ghost(rank), 1.0 + rank)
    assemble(V0, w)
    parts = [None] * world
    dist.all_gather_object(parts, (V0.own[rank], Pq.own[rank], yu, yp, w[: V0.n_own(rank)], V0.local_gid(rank)))
    if rank == 0:
        yg, wg, expect = np.zeros(nu + npp), np.zeros(nu), np.zeros(nu)
        for r, (vo, pown, a, b_, ww, lg) in enumerate(parts):
            yg[vo] = a; yg[nu + pown] = b_; wg[vo] = ww
            np.add.at(expect, lg, 1.0 + r)
        ref = sysd["K"] @ xg
        json.dump(dict(matvec_err=float(np.abs(yg - ref).max() / np.abs(ref).max()), assemble_err=float(np.abs(wg - expect).max()),
                       world=world, ghosts=[int(V0.n_ghost(0)), int(Pq.n_ghost(0))], mode="numpy_stokes"), open(out, "w"))
    dist.barrier()
    dist.destroy_process_group()


def main():
    mode, cells, nlev, out = sys.argv[1], tuple(int(c) for c in sys.argv[2].split("x")), int(sys.argv[3]), sys.argv[4]
    transport = sys.argv[5] if len(sys.argv) > 5 else "host"
    rep_from = int(sys.argv[6]) if len(sys.argv) > 6 and int(sys.argv[6]) > 0 else None
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = entry.import_package()
    from gridapsolvers_jl_amd import partition as pa, multigpu
    po = pkg.poisson
    d = len(cells)
    grid = pa.rank_grid(world, d)
    cg = pa.global_cells(cells, grid)
    maxiter, atol, rtol = 20, 1e-14, 1e-6
    order = int(os.environ.get("GMG_TEST_ORDER", "1"))
    smoother = os.environ.get("GMG_TEST_SMOOTHER", "jacobi")
    p_niter, p_omega = 4, 0.2
    depth = int(os.environ.get("GMG_TEST_DEPTH", "0"))      # > 0: partitioned levels >= 1 in the overlapping layout with that many ghost layers
    sub_from, sub_ranks = int(os.environ.get("GMG_TEST_SUB_FROM", "0")) or None, int(os.environ.get("GMG_TEST_SUB_RANKS", "0")) or None
    fdepth = int(os.environ.get("GMG_TEST_FINEST_DEPTH", "0"))   # > 0: the finest level in the overlapping layout too (separate Krylov operator)
    verdict = {}
    if mode == "numpy_stokes":
        return stokes_matvec_mode(cells[0], nlev, out, rank, world, dist, torch, pkg, po, pa)
    if mode == "gpu_stokes":
        return stokes_mode(cells[0], nlev, out, transport, rank, world, dist, torch, pkg, po, pa, multigpu)
    if mode == "gpu_block":
        pass
    elif mode == "numpy":
        local = pa.build_local_hierarchy(cg, nlev, grid, rank, order, None, rep_from, depth, smoother, finest_depth=fdepth,
                                         sub_from=sub_from, sub_ranks=sub_ranks)
        b = po.dirichlet_lift_rhs(cg, order)[local["levels"][0].own_gid]
        patches = None
        if smoother == "patch":
            patches = []
            for l in range(nlev - 1):
                Lc = local["levels"][l]
                if Lc is None:                                  # a level of a rank subset this rank is not part of
                    patches.append(None); continue
                Ag = po.poisson_matrix(local["cells"][l], order).to_scipy().tocsr()
                if getattr(Lc, "overlap", False):
                    pp, pl = Lc.ogeom.vertex_star_patches()
                    Al = Lc.A.to_scipy().tocsr()
                    Binv = [np.linalg.inv(Al[pl[pp[p]:pp[p + 1]]][:, pl[pp[p]:pp[p + 1]]].toarray()) if pp[p + 1] > pp[p] else None
                            for p in range(pp.size - 1)]
                    patches.append((pp, pl.astype(np.int64), Binv))
                    continue
                if Lc.replicated:
                    pp, pd = po.vertex_star_patches(local["cells"][l], order)
                    pl, pg = pd.astype(np.int64), pd.astype(np.int64)
                else:
                    pp, pl, pg = pa.local_vertex_star_patches(local["cells"][l], order, grid, rank)
                Binv = [np.linalg.inv(Ag[pg[pp[p]:pp[p + 1]]][:, pg[pp[p]:pp[p + 1]]].toarray()) if pp[p + 1] > pp[p] else None
                        for p in range(pp.size - 1)]
                patches.append((pp, pl.astype(np.int64), Binv))
            x, nit, hist = numpy_distributed_cg(local, rank, world, dist, torch, b, maxiter, atol, rtol, p_niter, p_omega, patches)
            verdict["exchanges"] = int(numpy_distributed_cg.last_exchanges)
        else:
            x, nit, hist = numpy_distributed_cg(local, rank, world, dist, torch, b, maxiter, atol, rtol)
            verdict["exchanges"] = int(numpy_distributed_cg.last_exchanges)
            verdict["redistributions"] = int(numpy_distributed_cg.last_redistributions)
        gid = local["levels"][0].own_gid
        verdict["hint_skips"] = (0 if os.environ.get("GMG_NO_OVERLAP_HINTS", "0") != "0" else
                                 int(sum(int(a) + int(b) for a, b in pa.overlap_hints(local, p_niter if smoother == "patch" else 10, smoother))))
    else:
        ndev = torch.cuda.device_count()
        dev = rank % max(ndev, 1)
        torch.cuda.set_device(dev)
        g = multigpu.DistributedGMG(cells, nlev, rank, world, device_id=dev, transport=transport, group=None, rep_from=rep_from,
                                    order=order, smoother=smoother, niter=(p_niter if smoother == "patch" else 10),
                                    omega=(p_omega if smoother == "patch" else 2.0 / 3.0), depth=depth, finest_depth=fdepth,
                                    sub_from=sub_from, sub_ranks=sub_ranks, cycle_type=os.environ.get("GMG_TEST_CYCLE", "v_cycle"),
                                    stream_rows=int(os.environ.get("GMG_TEST_STREAM_ROWS", "0")))
        verdict["streamed_levels"] = list(getattr(g, "streamed_levels", []))
        verdict["hint_skips"] = (0 if os.environ.get("GMG_NO_OVERLAP_HINTS", "0") != "0" else
                                 int(sum(int(a) + int(b) for a, b in getattr(g, "overlap_hints", []))))
        b = g.rhs_lin()
        x = np.zeros(g.n_own)
        # test hook: ONE rank behaves as if a one-launch smoothing pass had timed out in the first solve -- every rank must re-run it
        if os.environ.get("GMG_TEST_FORCE_TIMEOUT_RANK") is not None and int(os.environ["GMG_TEST_FORCE_TIMEOUT_RANK"]) == rank:
            import ctypes as C
            from gridapsolvers_jl_amd import abi
            abi.check(g.h, g._lib.gmg_set_option(g.h, b"persist_force_timeout", 1.0))
        ex0 = g.comm_stats()[0]
        log = g.cg_solve(b, x, maxiter, atol, rtol)
        verdict["exchanges"] = int(g.comm_stats()[0] - ex0)
        if os.environ.get("GMG_TEST_FORCE_TIMEOUT_RANK") is not None:
            import ctypes as C
            rr, act = C.c_int64(), C.c_int()
            g._lib.gmg_get_persist_retries(g.h, C.byref(rr), C.byref(act))
            allr = [None] * world
            dist.all_gather_object(allr, (int(rr.value), int(act.value)))
            verdict["persist_retries"] = [a[0] for a in allr]
            verdict["persist_active"] = [a[1] for a in allr]
        verdict["x_sha"] = __import__("hashlib").sha256(np.ascontiguousarray(x).tobytes()).hexdigest()
        if os.environ.get("GMG_TEST_REFRESH"):
            # numerical_setup! on EVERY level (GMGLinearSolvers.jl:260-297): all values doubled -- exact in binary floating point, so
            # solving A' x = 2 b must reproduce x -- through gmg_update_values with this rank's whole local rows (own and ghost columns
            # interleaved as they were handed over: a split stream routes them into the stream values and the boundary fix-up CSR)
            import ctypes as C
            from gridapsolvers_jl_amd import abi
            for l, Ll in enumerate(g.local["levels"]):
                v2 = np.ascontiguousarray(Ll.A.val * 2.0)
                abi.check(g.h, g._lib.gmg_update_values(g.h, l, C.c_void_p(v2.ctypes.data)))
            abi.check(g.h, g._lib.gmg_setup(g.h))
            x2 = np.zeros(g.n_own)
            log_r = g.cg_solve(2.0 * b, x2, maxiter, atol, rtol)
            mine = (int(log_r.num_iters), float(np.max(np.abs(x2 - x)) / np.max(np.abs(x))), bool(np.array_equal(x2, x)))
            allr = [None] * world
            dist.all_gather_object(allr, mine)
            verdict["refresh_iters"] = [a[0] for a in allr]
            verdict["refresh_dev"] = max(a[1] for a in allr)
            verdict["refresh_bitwise"] = all(a[2] for a in allr)
        nit, hist = log.num_iters, log.residuals[: log.num_iters + 1].copy()
        # also exercise device-pointer vectors + FGMRES
        xd = torch.zeros(g.n_own, dtype=torch.float64, device="cuda"); bd = torch.from_numpy(b).cuda(); torch.cuda.synchronize()
        log2 = g.fgmres_solve(bd, xd, m=5, maxiter=maxiter, atol=atol, rtol=rtol)
        verdict["fgmres_iters"] = int(log2.num_iters)
        verdict["fgmres_vs_cg"] = float(np.max(np.abs(xd.cpu().numpy() - x)))
        gid = g.local["levels"][0].own_gid
        g.close()
    if mode == "gpu_block":
        return block_mode(cells, nlev, out, transport, rank, world, dist, torch, pkg, po, pa, multigpu, grid, cg)
    # gather solution on rank 0
    parts = [None] * world
    dist.all_gather_object(parts, (gid, x, int(nit), hist.tolist()))
    if rank == 0:
        orc = entry.import_oracle()
        H = po.build_hierarchy(cg, nlev, order)
        bg = po.dirichlet_lift_rhs(cg, order)
        if smoother == "patch":
            sms = [orc.Smoother(orc.PATCH, p_niter, p_omega, *po.vertex_star_patches(c, order)) for c in H["ncells"][:-1]]
            go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sms, maxiter=1)
        else:
            go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], maxiter=1,
                         cycle={"v_cycle": orc.V_CYCLE, "w_cycle": orc.W_CYCLE, "f_cycle": orc.F_CYCLE}[os.environ.get("GMG_TEST_CYCLE", "v_cycle")])
        xo, nit_o, flag, hist_o = orc.cg_solve(H["mats"][0], bg, Pl=go, maxiter=maxiter, atol=atol, rtol=rtol)
        xg = np.zeros_like(xo)
        for gidq, xq, _, _ in parts:
            xg[gidq] = xq
        np.save(out + ".x.npy", xg)
        verdict.update(iters=int(nit), iters_oracle=int(nit_o), iters_all_equal=all(p[2] == nit for p in parts),
                       rel_err=float(np.linalg.norm(xg - xo) / np.linalg.norm(xo)),
                       hist_dev=float(np.max(np.abs(np.array(hist) - hist_o) / hist_o)) if len(hist) == len(hist_o) else 1.0,
                       l2_error_sq=float(po.l2_error_sq(cg, order, xg)), world=world, grid=list(grid), mode=mode)
        json.dump(verdict, open(out, "w"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    if os.environ.get("GMG_TEST_THREAD_RANKS"):          # every rank a thread of this process (thread_ranks.py)
        import thread_ranks
        thread_ranks.run(int(os.environ["WORLD_SIZE"]), lambda r: main())
    else:
        main()
