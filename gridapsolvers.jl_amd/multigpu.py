"""Multi-GPU driver: one process per GPU, PartitionedArrays-style row partition.

`DistributedGMG` is the distributed counterpart of `solvers.GMGNumericalSetup`: it builds this
rank's local operators (partition.py), creates the native handle, connects the ranks
(RCCL over xGMI, communicator seeded through torch.distributed; or the host-staged
callback transport used by the tests when several ranks share one GPU) and uploads the
exchange plans.  Reference analogue: `with_mpi()` + `CartesianModelHierarchy(parts,np_per_level,...)`
+ `PSparseMatrix`/`PVector` (test/LinearSolvers/mpi/GMGTests.jl:5-8, GMGTests.jl:100-144).

Weak scaling: every rank owns `cells_per_rank` cells per direction on the finest level, the
global mesh is `cells_per_rank * rank_grid`.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import time

import numpy as np

from . import abi, partition as pa, poisson as po
from .solvers import ChebyshevSmoother, ConvergenceLog, GaussSeidelSmoother, JacobiLinearSolver, _vec


def rccl_path():
    """Prefer the librccl.so already loaded with PyTorch-ROCm (one RCCL per process)."""
    try:
        import torch
        p = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        if os.path.exists(p):
            return p
    except Exception:
        pass
    return "/opt/rocm/lib/librccl.so.1"


class _HostTransport:
    """consistent! / all-reduce through torch.distributed on CPU tensors (gloo)."""

    def __init__(self, group):
        import torch
        import torch.distributed as dist
        self.torch, self.dist, self.group = torch, dist, group

        def exchange(ctx, nnbr, nbr_rank, sendbuf, snd_ptr, recvbuf, rcv_ptr):
            ops, keep = [], []
            for k in range(nnbr):
                q = int(nbr_rank[k])
                s0, s1 = int(snd_ptr[k]), int(snd_ptr[k + 1])
                r0, r1 = int(rcv_ptr[k]), int(rcv_ptr[k + 1])
                if r1 > r0:
                    t = torch.from_numpy(np.ctypeslib.as_array(recvbuf, shape=(int(rcv_ptr[nnbr]),))[r0:r1])
                    ops.append(dist.P2POp(dist.irecv, t, self._global(q), group=self.group)); keep.append(t)
                if s1 > s0:
                    t = torch.from_numpy(np.ctypeslib.as_array(sendbuf, shape=(int(snd_ptr[nnbr]),))[s0:s1].copy())
                    ops.append(dist.P2POp(dist.isend, t, self._global(q), group=self.group)); keep.append(t)
            if ops:
                for w in dist.batch_isend_irecv(ops):
                    w.wait()

        def allreduce(ctx, vals, n):
            t = torch.from_numpy(np.ctypeslib.as_array(vals, shape=(n,)))
            dist.all_reduce(t, group=self.group)

        self.exchange_cb = abi.HOST_EXCHANGE_FN(exchange)
        self.allreduce_cb = abi.HOST_ALLREDUCE_FN(allreduce)

    def _global(self, q):
        return self.dist.get_global_rank(self.group, q) if self.group is not None else q


class _AloneTransport:
    """Measurement only (tools/rank_alone.py): ONE rank of an N-rank partition runs by itself -- every halo it would receive is zero,
    every scalar all-reduce returns N times its own contribution (so that joint decisions pass), vector all-reduces return the rank's
    own part.  The numbers it computes mean nothing; the kernels it launches, their shapes and their order are exactly those of
    that rank in the N-rank run, with the GPU to itself: the communication-free part of an iteration."""

    def __init__(self, world):
        def exchange(ctx, nnbr, nbr_rank, sendbuf, snd_ptr, recvbuf, rcv_ptr):
            n = int(rcv_ptr[nnbr])
            if n > 0:
                np.ctypeslib.as_array(recvbuf, shape=(n,))[:] = 0.0

        def allreduce(ctx, vals, n):
            if n == 1:
                vals[0] = vals[0] * world

        self.exchange_cb = abi.HOST_EXCHANGE_FN(exchange)
        self.allreduce_cb = abi.HOST_ALLREDUCE_FN(allreduce)


class _LoopbackTransport:
    """Host-staged counterpart of gmg_comm_set_loopback: message k of a plan goes from send segment k to receive segment k of the
    same rank; all-reduces over the one real rank are the identity.  The bit-for-bit reference of the RCCL loopback run."""

    def __init__(self):
        def exchange(ctx, nnbr, nbr_rank, sendbuf, snd_ptr, recvbuf, rcv_ptr):
            ns, nr = int(snd_ptr[nnbr]), int(rcv_ptr[nnbr])
            if nr == 0:
                return
            s, r = np.ctypeslib.as_array(sendbuf, shape=(ns,)), np.ctypeslib.as_array(recvbuf, shape=(nr,))
            for k in range(nnbr):
                s0, s1, r0, r1 = int(snd_ptr[k]), int(snd_ptr[k + 1]), int(rcv_ptr[k]), int(rcv_ptr[k + 1])
                assert s1 - s0 == r1 - r0, "loopback: message k must have the same length on both sides"
                r[r0:r1] = s[s0:s1]

        def allreduce(ctx, vals, n):
            pass

        self.exchange_cb = abi.HOST_EXCHANGE_FN(exchange)
        self.allreduce_cb = abi.HOST_ALLREDUCE_FN(allreduce)


class DistributedGMG:
    """Distributed numerical setup of CG/FGMRES + GMG on the structured Poisson hierarchy."""

    def __init__(self, cells_per_rank, nlevels, rank, world, device_id=0, transport="rccl", group=None,
                 order=1, niter=10, omega=2.0 / 3.0, mode="preconditioner", cycle_type="v_cycle",
                 gmg_maxiter=1, gmg_atol=1e-14, gmg_rtol=1e-8, local_hierarchy=None, lengths=None, rep_from=None,
                 smoother="jacobi", depth=None, patch_tables=None, pcorr_tables=None, cells_global=None, options=None,
                 stream_rows=0, finest_depth=0, sub_from=None, sub_ranks=None, gs_orders=None, loopback_rows=None, chebyshev=None):
        """smoother = "jacobi": Richardson(Jacobi, niter, omega); "patch": Richardson(PatchSolver, niter, omega) with the
        vertex-star patches OWNED by this rank (partition.local_vertex_star_patches) and caller-assembled patch matrices --
        a rank's local matrix has the owned rows only, so the blocks of patches reaching into ghost dofs come from the
        driver, as the reference assembles them from the solver's weak form on the local (ghosted) mesh
        (PatchSolvers.jl:137-150).
        smoother = a solvers.GaussSeidelSmoother / SymGaussSeidelSmoother(...) object: that smoother (its niter, omega, type and ordering;
        the arguments niter / omega are not used) pre and post on every smoothed level, as rank-block Gauss-Seidel on the partitioned
        levels -- every rank sweeps the own x own block of its local matrix, r -= A dx is the distributed product -- and as global
        sweeps on the replicated ones.  "natural" and "multicolor" hold per rank block; a given order is per level and per rank: a
        list indexed by level, gs_orders, whose entry l is this rank's permutation of the level's owned rows (None: the smoother's
        ordering; a folded partition takes the permutation of the folded own block; a replicated level one of its global rows).  Needs the own | ghost layout: depth / finest_depth other than None / 0 raise
        ValueError.
        chebyshev = a mapping of ChebyshevSmoother's keyword arguments (degree, lambda_max, lambda_min, eig_ratio, eig_safety, eig_steps,
        eig_method; {} = its defaults): ChebyshevSmoother(M, ...) pre and post on every smoothed level over the M that `smoother` names
        ("jacobi": JacobiLinearSolver, "patch": PatchSolver); niter / omega are then unused.  On the partitioned levels the recurrence
        runs on the owned rows with the distributed product, on the replicated ones as on one GPU; an estimated lambda_max comes from
        all-reduced scalars (chebyshev_info).  Needs the own | ghost layout on all ranks: together with a GaussSeidelSmoother, with
        depth / finest_depth other than None / 0 or with sub_from it raises ValueError.
        local_hierarchy: ready-made local operators (dict like partition.build_local_hierarchy's: levels = objects with A, P, R, n_own,
        n_ghost, nbr_rank, snd_ptr, snd_idx, rcv_ptr, replicated; rep_from; rep_gid) -- e.g. from dpartition for the vector-valued
        Stokes velocity hierarchy; then patch_tables[l] = (patch_ptr, dofs, blocks) supplies the smoother's patches per level
        (local numbering + caller-assembled matrices on partitioned levels, global numbering and blocks=None on replicated ones)
        and pcorr_tables[l] = (patch_ptr, local dofs, G_local or None) a patch-corrected prolongation
        (PatchProlongationOperator, PatchTransferOperators.jl:153-172) with its rhs form.
        depth: ghost layers of the OVERLAPPING layout on the partitioned levels >= 1 (int or per-level list; None / 0 = every level in
        the own | ghost layout): one halo exchange per `depth` sweeps instead of one per sweep (gmg_set_partition_overlap).
        finest_depth > 0: the finest level in the overlapping layout as well -- the Krylov solver keeps the caller's own | ghost vectors
        and its own finest operator (GMG_LEVEL_KRYLOV: gmg_set_matrix / gmg_set_partition / gmg_set_krylov_map), the preconditioner's
        level 0 smooths in the extended-box numbering with one exchange per `finest_depth` sweeps.
        sub_from / sub_ranks: the partitioned levels sub_from .. rep_from-1 on the first `sub_ranks` ranks only (np_per_level /
        redistribute! of the reference; gmg_set_redistribution: glued partition on all ranks + the subset's, two p2p plans) -- a
        capability: the communication model never prefers it on this hardware.
        loopback_rows (loopback transports): the owned rows of every folded rank on level 0 (gmg_comm_set_loopback_rows) -- the dot
        products and norms of CG are then reduced rank by rank and added in rank order, the scalars of the true W-rank run.
        stream_rows > 0: the operators of the levels that are laid out like a single-GPU level -- overlapping layout, replicated levels
        -- are handed over in blocks of that many rows (gmg_set_operator_rows): the library keeps their row-pattern form only, never
        a CSR copy (what a per-rank assembler that produces its rows plane by plane would do)."""
        import torch.distributed as dist
        gs = smoother if isinstance(smoother, GaussSeidelSmoother) else None
        cheb = None
        if chebyshev is not None:
            if gs is not None:
                raise ValueError("chebyshev goes with smoother = \"jacobi\" or \"patch\": there is no Chebyshev iteration over a Gauss-Seidel smoother")
            if (depth is not None and np.any(np.asarray(depth) != 0)) or finest_depth:
                raise ValueError("a Chebyshev smoother needs the own | ghost layout on every partitioned level: depth / finest_depth must be None / 0")
            if sub_from is not None:
                raise ValueError("a Chebyshev smoother does not run on the levels of a rank subset: sub_from must be None")
            cheb = ChebyshevSmoother(JacobiLinearSolver(), **dict(chebyshev))   # (validation only: the errors are the constructor's)
        if gs is not None:
            if (depth is not None and np.any(np.asarray(depth) != 0)) or finest_depth:
                raise ValueError("a Gauss-Seidel smoother needs the own | ghost layout on every partitioned level: depth / finest_depth must be None / 0")
            if not isinstance(gs.ordering, str):
                raise ValueError("a given ordering is per level and per rank: pass gs_orders=[order of level 0, order of level 1, ...]")
            if gs_orders is not None:
                if len(gs_orders) > nlevels - 1:
                    raise ValueError("gs_orders: one entry per smoothed level at the most")
                gs_orders = [None if o is None else GaussSeidelSmoother._check_ordering(o) for o in gs_orders]
                if any(isinstance(o, str) for o in gs_orders):
                    raise ValueError("gs_orders: every entry is None or a 1-D integer array")
        elif gs_orders is not None or not isinstance(smoother, str):
            raise ValueError('smoother must be "jacobi", "patch" or a GaussSeidelSmoother (gs_orders goes with the latter)')
        lib = abi.load()
        self._lib, self.rank, self.world = lib, rank, world
        d = len(cells_per_rank)
        self.grid = pa.rank_grid(world, d)
        self.cells_global = tuple(cells_global) if cells_global is not None else pa.global_cells(cells_per_rank, self.grid)
        self._patch_tables, self._pcorr_tables = patch_tables, pcorr_tables
        t0 = time.perf_counter()
        # `lengths` = domain extents; the weak-scaling bench uses (px,py,pz) so that cells stay cubes
        # (an anisotropic mesh would change the iteration count with the rank grid)
        self.lengths = lengths
        self.local = local_hierarchy or pa.build_local_hierarchy(self.cells_global, nlevels, self.grid, rank, order, lengths, rep_from,
                                                                  depth, "jacobi" if gs is not None else smoother, finest_depth=finest_depth, sub_from=sub_from,
                                                                  sub_ranks=sub_ranks)
        self.t_assembly = time.perf_counter() - t0
        self.order = order
        h = C.c_void_p()
        abi.check(None, lib.gmg_create(C.byref(h), nlevels, device_id))
        self.h = h
        self.transport = transport
        self._keep = []
        for k, v in (options or {}).items():         # per-handle layout / schedule policy (gmg_set_option), before anything is set
            abi.check(h, lib.gmg_set_option(h, str(k).encode(), float(v)))
        if world > 1:
            if transport == "rccl":
                path = rccl_path().encode()
                uid = C.create_string_buffer(128)
                if rank == 0:
                    abi.check(None, lib.gmg_comm_unique_id(path, uid))
                blob = [bytes(uid.raw) if rank == 0 else None]
                dist.broadcast_object_list(blob, src=0, group=group)
                abi.check(h, lib.gmg_comm_init_rccl(h, path, blob[0], rank, world))
            elif transport == "rccl_loopback":
                # ONE real rank, a partition folded onto it (partition.fold_ranks): RCCL's own unique id, a communicator of one rank
                path = rccl_path().encode()
                uid = C.create_string_buffer(128)
                abi.check(None, lib.gmg_comm_unique_id(path, uid))
                abi.check(h, lib.gmg_comm_init_rccl(h, path, bytes(uid.raw), 0, 1))
                abi.check(h, lib.gmg_comm_set_loopback(h, world))
            elif transport == "host_loopback":
                self._host = _LoopbackTransport()
                abi.check(h, lib.gmg_comm_init_host(h, 0, 1, C.cast(self._host.exchange_cb, C.c_void_p),
                                                    C.cast(self._host.allreduce_cb, C.c_void_p), None))
                abi.check(h, lib.gmg_comm_set_loopback(h, world))
            elif transport in ("host", "alone"):
                self._host = _HostTransport(group) if transport == "host" else _AloneTransport(world)
                abi.check(h, lib.gmg_comm_init_host(h, rank, world, C.cast(self._host.exchange_cb, C.c_void_p),
                                                    C.cast(self._host.allreduce_cb, C.c_void_p), None))
            else:
                raise ValueError("transport must be 'rccl', 'host', 'alone', 'rccl_loopback' or 'host_loopback'")
        if loopback_rows is not None:
            if transport not in ("rccl_loopback", "host_loopback"):
                raise ValueError("loopback_rows goes with the loopback transports")
            rows = np.ascontiguousarray(loopback_rows, dtype=np.int64)
            abi.check(h, lib.gmg_comm_set_loopback_rows(h, C.c_void_p(rows.ctypes.data), rows.size))
        levels = self.local["levels"]
        for l, L in enumerate(levels):
            if L is None:                                     # a level of a rank subset this rank is not part of
                continue
            if world > 1 and not L.replicated:
                if not hasattr(L, "overlap"):
                    L.overlap = False
                nbr = np.ascontiguousarray(L.nbr_rank, dtype=np.int32)
                sp, si, rp = (np.ascontiguousarray(a, dtype=np.int64) for a in (L.snd_ptr, L.snd_idx, L.rcv_ptr))
                self._keep += [nbr, sp, si, rp]
                if L.overlap:
                    ri = np.ascontiguousarray(L.rcv_idx, dtype=np.int64)
                    self._keep.append(ri)
                    abi.check(h, lib.gmg_set_partition_overlap(h, l, L.n_local, L.n_ghost, L.depth, nbr.size, C.c_void_p(nbr.ctypes.data),
                                                               C.c_void_p(sp.ctypes.data), C.c_void_p(si.ctypes.data),
                                                               C.c_void_p(rp.ctypes.data), C.c_void_p(ri.ctypes.data)))
                else:
                    abi.check(h, lib.gmg_set_partition(h, l, L.n_own, L.n_ghost, nbr.size, C.c_void_p(nbr.ctypes.data),
                                                       C.c_void_p(sp.ctypes.data), C.c_void_p(si.ctypes.data),
                                                       C.c_void_p(rp.ctypes.data)))
            # single-GPU-like levels: overlapping layout or replicated (the coarsest level needs its matrix whole: dense inverse)
            streamable = stream_rows > 0 and (L.replicated or getattr(L, "overlap", False) or world == 1) and l < nlevels - 1
            self.streamed_levels = getattr(self, "streamed_levels", []) + ([l] if streamable else [])
            # an own | ghost level: the library splits every block into the own x own part (stream) and the ghost columns (small CSR)
            split_stream = stream_rows > 0 and world > 1 and not L.replicated and not getattr(L, "overlap", False) and l < nlevels - 1
            if split_stream:
                self.streamed_levels.append(l)
            if streamable or split_stream:
                self._stream(abi.OP_A, l, L.A, stream_rows)
            else:
                self._set(lib.gmg_set_matrix, l, L.A)
            if l < nlevels - 1:
                nxt = levels[l + 1]
                t_stream = streamable and nxt is not None and (nxt.replicated or getattr(nxt, "overlap", False) or world == 1)
                if t_stream:
                    self._stream(abi.OP_P, l, L.P, stream_rows)
                    self._stream(abi.OP_R, l, L.R, stream_rows)
                else:
                    self._set(lib.gmg_set_prolongation, l, L.P)
                    self._set(lib.gmg_set_restriction, l, L.R)
                if gs is not None:
                    abi.check(h, lib.gmg_set_smoother_gauss_seidel(h, l, abi.PRE_AND_POST, gs.niter, gs.omega, GaussSeidelSmoother._TYPES[gs.type]))
                    o = gs_orders[l] if gs_orders is not None and l < len(gs_orders) and gs_orders[l] is not None else gs.ordering
                    if isinstance(o, str):
                        if o != "natural":
                            abi.check(h, lib.gmg_set_gs_ordering(h, l, GaussSeidelSmoother._ORDERINGS[o], None, 0))
                    else:
                        abi.check(h, lib.gmg_set_gs_ordering(h, l, abi.GS_ORDER_GIVEN, C.c_void_p(o.ctypes.data), o.size))
                elif smoother == "patch":
                    self._set_patch_smoother(l, L, niter, omega)
                else:
                    abi.check(h, lib.gmg_set_smoother_jacobi(h, l, abi.PRE_AND_POST, niter, omega))
                if cheb is not None:
                    abi.check(h, lib.gmg_set_smoother_chebyshev(h, l, abi.PRE_AND_POST, cheb.degree, 0.0 if cheb.lambda_min is None else cheb.lambda_min,
                                                                0.0 if cheb.lambda_max is None else cheb.lambda_max, cheb.eig_steps, cheb.eig_ratio,
                                                                cheb.eig_safety))
                    if cheb.eig_method != "power":
                        abi.check(h, lib.gmg_set_chebyshev_eig_method(h, l, abi.PRE_AND_POST, cheb._EIG_METHODS[cheb.eig_method]))
                if pcorr_tables is not None and pcorr_tables[l] is not None:
                    pp, pl, G = pcorr_tables[l]
                    pp64, pl64 = np.ascontiguousarray(pp, dtype=np.int64), np.ascontiguousarray(pl, dtype=np.int64)
                    self._keep += [pp64, pl64]
                    abi.check(h, lib.gmg_set_prolongation_patch_correction(h, l, abi.PATCH_LU, pp64.size - 1, C.c_void_p(pp64.ctypes.data),
                                                                           C.c_void_p(pl64.ctypes.data), 0, 8))
                    if G is not None:
                        gp, gi = np.ascontiguousarray(G.ptr, dtype=np.int64), np.ascontiguousarray(G.idx, dtype=np.int64)
                        abi.check(h, lib.gmg_set_prolongation_patch_correction_rhs(h, l, G.shape[0], G.nnz, C.c_void_p(gp.ctypes.data),
                                                                                   C.c_void_p(gi.ctypes.data), C.c_void_p(G.val.ctypes.data), abi.CSR, 0, 8))
        if world > 1 and (local_hierarchy is None or self.local.get("structured")) and "order" in self.local:
            # transfer exchanges the halo geometry makes unnecessary (consistent!(r) before the restriction, consistent!(dxh) before r -= A dxh)
            # (the library is told the geometry -- layers, layers per sweep, reach of R -- and derives the first skip per pass itself;
            # overlap_hints() is the same rule evaluated here for this niter: what the bench line reports)
            geom_smoother = "jacobi" if gs is not None else smoother   # (a Gauss-Seidel hierarchy has no overlapping level: no hints)
            self.overlap_hints = pa.overlap_hints(self.local, niter, geom_smoother)
            for l, (lay, per, rr, sd) in enumerate(pa.overlap_geometry(self.local, geom_smoother)):
                if lay > 0 and not int(os.environ.get("GMG_NO_OVERLAP_HINTS", "0")):
                    abi.check(h, lib.gmg_set_partition_overlap_hints(h, l, lay, per, rr, int(sd)))
        sub = self.local.get("sub") if world > 1 else None
        if sub is not None:
            tp, fp = abi.RedistPlan.from_dict(sub["to_sub"], self._keep), abi.RedistPlan.from_dict(sub["from_sub"], self._keep)
            abi.check(h, lib.gmg_set_redistribution(h, sub["sub_from"], int(sub["member"]), sub["n_glue_own"], sub["n_glue_ghost"],
                                                    C.byref(tp), C.byref(fp)))
        K = self.local.get("krylov") if world > 1 else None
        if K is not None:
            # finest level in the overlapping layout: the Krylov operator in the caller's own | ghost numbering + the owned entries' places
            nbr = np.ascontiguousarray(K.nbr_rank, dtype=np.int32)
            sp, si, rp, o2l = (np.ascontiguousarray(a, dtype=np.int64) for a in (K.snd_ptr, K.snd_idx, K.rcv_ptr, K.own_idx))
            self._keep += [nbr, sp, si, rp, o2l]
            abi.check(h, lib.gmg_set_partition(h, abi.LEVEL_KRYLOV, K.n_own, K.n_ghost, nbr.size, C.c_void_p(nbr.ctypes.data),
                                               C.c_void_p(sp.ctypes.data), C.c_void_p(si.ctypes.data), C.c_void_p(rp.ctypes.data)))
            self._set(lib.gmg_set_matrix, abi.LEVEL_KRYLOV, K.A)
            abi.check(h, lib.gmg_set_krylov_map(h, C.c_void_p(o2l.ctypes.data), o2l.size))
        if world > 1:
            gid = self.local["rep_gid"]
            self._keep.append(gid)
            abi.check(h, lib.gmg_set_replication(h, self.local["rep_from"], C.c_void_p(gid.ctypes.data), gid.size))
        modes = {"preconditioner": abi.MODE_PRECONDITIONER, "solver": abi.MODE_SOLVER}
        cycles = {"v_cycle": abi.V_CYCLE, "w_cycle": abi.W_CYCLE, "f_cycle": abi.F_CYCLE}
        abi.check(h, lib.gmg_set_options(h, modes[mode], cycles[cycle_type], gmg_maxiter, gmg_atol, gmg_rtol))
        t0 = time.perf_counter()
        abi.check(h, lib.gmg_setup(h))
        self.t_setup = time.perf_counter() - t0
        self.n_own = levels[0].n_own
        self.n_global = po.level_sizes(self.cells_global, order) if (local_hierarchy is None or self.local.get("structured")) else None
        self.nnz_local = levels[0].A.nnz

    def _set_patch_smoother(self, l, L, niter, omega):
        lib, h = self._lib, self.h
        if self._patch_tables is not None:                   # caller-made tables (generic hierarchies, e.g. the Stokes velocity block)
            pp, pd, blocks = self._patch_tables[l]
            pp64, pd64 = np.ascontiguousarray(pp, dtype=np.int64), np.ascontiguousarray(pd, dtype=np.int64)
            self._keep += [pp64, pd64]
            if blocks is None:
                abi.check(h, lib.gmg_set_smoother_patch(h, l, abi.PRE_AND_POST, niter, omega, abi.PATCH_LU, pp64.size - 1,
                                                        C.c_void_p(pp64.ctypes.data), C.c_void_p(pd64.ctypes.data), 0, 8))
            else:
                blocks = np.ascontiguousarray(blocks)
                self._keep.append(blocks)
                abi.check(h, lib.gmg_set_smoother_patch_matrices(h, l, abi.PRE_AND_POST, niter, omega, abi.PATCH_LU, pp64.size - 1,
                                                                 C.c_void_p(pp64.ctypes.data), C.c_void_p(pd64.ctypes.data), None, 0, 8,
                                                                 C.c_void_p(blocks.ctypes.data), 0, None))
            return
        cells_l = self.local["cells"][l]
        if getattr(L, "overlap", False):
            # overlapping layout: every vertex star inside the extended box, blocks A[p,p] from the local matrix (exact there): no
            # caller-assembled matrices, no assemble! -- the level is a single-GPU level between two exchanges
            pp, pd = L.ogeom.vertex_star_patches()
            self._keep += [pp, pd]
            abi.check(h, lib.gmg_set_smoother_patch(h, l, abi.PRE_AND_POST, niter, omega, abi.PATCH_LU, pp.size - 1,
                                                    C.c_void_p(pp.ctypes.data), C.c_void_p(pd.ctypes.data), 0, 8))
            return
        if L.replicated or self.world == 1:
            pp, pd = po.vertex_star_patches(cells_l, self.order)
            pd64 = pd.astype(np.int64)
            self._keep += [pp, pd64]
            abi.check(h, lib.gmg_set_smoother_patch(h, l, abi.PRE_AND_POST, niter, omega, abi.PATCH_LU, pp.size - 1,
                                                    C.c_void_p(pp.ctypes.data), C.c_void_p(pd64.ctypes.data), 0, 8))
            return
        pp, pl, pg = pa.local_vertex_star_patches(cells_l, self.order, self.grid, self.rank)
        Ag = po.poisson_matrix(cells_l, self.order, self.lengths).to_scipy().tocsr()   # driver-side assembly of the patch matrices
        blocks = [Ag[pg[pp[p]:pp[p + 1]]][:, pg[pp[p]:pp[p + 1]]].toarray().reshape(-1, order="F") for p in range(pp.size - 1)]
        blocks = np.ascontiguousarray(np.concatenate(blocks)) if blocks else np.zeros(0)
        pl64 = pl.astype(np.int64)
        self._keep += [pp, pl64, blocks]
        abi.check(h, lib.gmg_set_smoother_patch_matrices(h, l, abi.PRE_AND_POST, niter, omega, abi.PATCH_LU, pp.size - 1,
                                                         C.c_void_p(pp.ctypes.data), C.c_void_p(pl64.ctypes.data), None, 0, 8,
                                                         C.c_void_p(blocks.ctypes.data), 0, None))

    def _stream(self, op, l, M, block):
        """the rows of M in consecutive blocks (gmg_set_operator_rows); every block is dropped after the call"""
        n = M.shape[0]
        for r0 in range(0, n, block):
            r1 = min(n, r0 + block)
            k0, k1 = int(M.ptr[r0]), int(M.ptr[r1])
            ptr = (M.ptr[r0:r1 + 1] - k0).astype(np.int64)
            idx = np.ascontiguousarray(M.idx[k0:k1], dtype=np.int64)
            val = np.ascontiguousarray(M.val[k0:k1])
            abi.check(self.h, self._lib.gmg_set_operator_rows(self.h, l, op, M.shape[0], M.shape[1], r0, r1 - r0, C.c_void_p(ptr.ctypes.data),
                                                              C.c_void_p(idx.ctypes.data), C.c_void_p(val.ctypes.data), 0, 8))

    def _set(self, fn, l, M):
        if M.nnz < 2 ** 31 - 1:            # int32 columns as they are, the (short) pointer array narrowed to match
            ptr = M.ptr.astype(np.int32)
            abi.check(self.h, fn(self.h, l, M.shape[0], M.shape[1], M.nnz, C.c_void_p(ptr.ctypes.data),
                                 C.c_void_p(M.idx.ctypes.data), C.c_void_p(M.val.ctypes.data), abi.CSR, 0, 4))
            return
        idx64 = M.idx.astype(np.int64)
        abi.check(self.h, fn(self.h, l, M.shape[0], M.shape[1], M.nnz, C.c_void_p(M.ptr.ctypes.data),
                             C.c_void_p(idx64.ctypes.data), C.c_void_p(M.val.ctypes.data), abi.CSR, 0, 8))

    # -- right-hand sides ------------------------------------------------------------------
    def _nodal_u(self, gid):
        """u = x1 + x2 at the free dofs `gid` (global lexicographic ids, x fastest) -- from coordinates, no global arrays"""
        d = len(self.cells_global)
        nf = [self.order * c - 1 for c in self.cells_global]
        Ls = po._lengths(self.lengths, d)
        i = gid % nf[0]
        j = (gid // nf[0]) % nf[1]
        h0, h1 = Ls[0] / (self.order * self.cells_global[0]), Ls[1] / (self.order * self.cells_global[1])
        return (i + 1) * h0 + (j + 1) * h1

    def rhs_lin(self):
        """Owned part of the Dirichlet-lift rhs of u = x1 + x2 (reference test problem, f = 0): u is in the FE space, so
        A_ff u_f + A_fd u_d = 0 and b = -A_fd u_d = A_ff u_f -- evaluated with this rank's local rows on the nodal values of its
        [own | ghost] dofs; nothing of global size is formed (576^3 nodes at 8 x 288^3)."""
        L0 = self.local.get("krylov") or self.local["levels"][0]   # (the own | ghost rows: the Krylov operator when level 0 overlaps)
        u = self._nodal_u(np.concatenate([L0.own_gid, L0.ghost_gid]))
        return np.ascontiguousarray(L0.A.matvec(u))

    def exact_own(self):
        return np.ascontiguousarray(self._nodal_u(self.local["levels"][0].own_gid))

    # -- solves ----------------------------------------------------------------------------
    def cg_solve(self, b, x, maxiter=20, atol=1e-14, rtol=1e-6, flexible=False):
        log = ConvergenceLog("CG", maxiter, atol, rtol)
        pb, ms, _kb = _vec(b, self.n_own)
        px, ms2, _kx = _vec(x, self.n_own, writable=True)
        assert ms == ms2
        res = abi.Result()
        hist = np.zeros(maxiter + 1)
        abi.check(self.h, self._lib.gmg_cg_solve(self.h, pb, px, ms, maxiter, atol, rtol, int(flexible), 1,
                                                 C.byref(res), C.c_void_p(hist.ctypes.data), hist.size))
        log._fill(res, hist)
        return log

    def minres_solve(self, b, x, maxiter=20, atol=1e-14, rtol=1e-6):
        """MINRESSolver(;Pl=this GMG) on the partitioned system (MINRESSolvers.jl:75-148)"""
        log = ConvergenceLog("MINRES", maxiter, atol, rtol)
        pb, ms, _kb = _vec(b, self.n_own)
        px, ms2, _kx = _vec(x, self.n_own, writable=True)
        assert ms == ms2
        res = abi.Result()
        hist = np.zeros(maxiter + 1)
        abi.check(self.h, self._lib.gmg_minres_solve(self.h, pb, px, ms, maxiter, atol, rtol, 1,
                                                     C.byref(res), C.c_void_p(hist.ctypes.data), hist.size))
        log._fill(res, hist)
        return log

    def gmres_solve(self, b, x, m=5, maxiter=20, atol=1e-14, rtol=1e-6, restart=False, m_add=1, side="right"):
        """GMRESSolver(m; Pr=this GMG) (side="right") or GMRESSolver(m; Pl=this GMG) ("left") on the partitioned system
        (GMRESSolvers.jl:132-210); with a communicator the dots are all-reduced (the unfused Arnoldi sequence)"""
        log = ConvergenceLog("GMRES", maxiter, atol, rtol)
        pb, ms, _kb = _vec(b, self.n_own)
        px, ms2, _kx = _vec(x, self.n_own, writable=True)
        assert ms == ms2 and side in ("right", "left")
        res = abi.Result()
        hist = np.zeros(maxiter + 1)
        abi.check(self.h, self._lib.gmg_gmres_solve(self.h, pb, px, ms, m, int(restart), m_add, maxiter, atol, rtol,
                                                    int(side == "right"), int(side == "left"),
                                                    C.byref(res), C.c_void_p(hist.ctypes.data), hist.size))
        log._fill(res, hist)
        return log

    def set_stream(self, stream=None):
        """gmg_set_stream: the handle's work on the caller's HIP stream (torch.cuda.Stream, integer hipStream_t, None = its own)"""
        abi.check(self.h, self._lib.gmg_set_stream(self.h, abi.stream_arg(stream)))

    def fgmres_solve(self, b, x, m=5, maxiter=20, atol=1e-14, rtol=1e-6, restart=False, m_add=1):
        log = ConvergenceLog("FGMRES", maxiter, atol, rtol)
        pb, ms, _kb = _vec(b, self.n_own)
        px, ms2, _kx = _vec(x, self.n_own, writable=True)
        assert ms == ms2
        res = abi.Result()
        hist = np.zeros(maxiter + 1)
        abi.check(self.h, self._lib.gmg_fgmres_solve(self.h, pb, px, ms, m, int(restart), m_add, maxiter, atol, rtol, 1,
                                                     C.byref(res), C.c_void_p(hist.ctypes.data), hist.size))
        log._fill(res, hist)
        return log

    def apply(self, r, z, maxiter=1):
        log = ConvergenceLog("GMG", maxiter, 1e-14, 1e-8)
        pr, ms, _k1 = _vec(r, self.n_own)
        pz, ms2, _k2 = _vec(z, self.n_own, writable=True)
        res = abi.Result()
        hist = np.zeros(maxiter + 1)
        abi.check(self.h, self._lib.gmg_apply(self.h, pr, pz, ms, C.byref(res), C.c_void_p(hist.ctypes.data), hist.size))
        log._fill(res, hist)
        return log

    def profile(self, lev=0, enable=True):
        abi.check(self.h, self._lib.gmg_profile_enable(self.h, lev, 1 if enable else 0))

    def kernel_stats(self):
        st = abi.KernelStats()
        abi.check(self.h, self._lib.gmg_get_kernel_stats(self.h, C.byref(st)))
        return dict(launches=st.launches, total_ms=st.total_ms, alg_bytes=st.alg_bytes, rows=st.rows, nnz=st.nnz,
                    layout_bytes=st.layout_bytes)

    def comm_stats(self):
        """(halo exchanges, all-reduces) this rank's handle has issued so far"""
        a, b = C.c_int64(0), C.c_int64(0)
        abi.check(self.h, self._lib.gmg_get_comm_stats(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def sweep_signature(self, lev=0):
        buf = C.create_string_buffer(256)
        abi.check(self.h, self._lib.gmg_sweep_signature(self.h, lev, buf, 256))
        return buf.value.decode()

    def chebyshev_info(self, level=0, which="pre"):
        """gmg_get_chebyshev_info / gmg_get_chebyshev_eig of a slot (which = "pre" / "post"), as GMGNumericalSetup.chebyshev_info ->
        dict(degree, lambda_est (NaN where the bounds were given), lambda_min, lambda_max, eig_steps, eig_method, eig_steps_done).  On a
        partitioned level lambda_est comes from scalars reduced over the ranks: the same value on every rank, but one that depends on the
        partition (the start vector is indexed by the rank's own rows)."""
        if which not in ("pre", "post"):
            raise ValueError('which must be "pre" or "post"')
        w = abi.PRE if which == "pre" else abi.POST
        deg, steps, meth, done = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        v = [C.c_double(0.0) for _ in range(3)]
        abi.check(self.h, self._lib.gmg_get_chebyshev_info(self.h, level, w, C.byref(deg), C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(steps)))
        abi.check(self.h, self._lib.gmg_get_chebyshev_eig(self.h, level, w, C.byref(meth), C.byref(done)))
        return dict(degree=deg.value, lambda_est=v[0].value, lambda_min=v[1].value, lambda_max=v[2].value, eig_steps=steps.value,
                    eig_method=("power", "lanczos")[meth.value], eig_steps_done=done.value)

    def gs_schedule(self, level=0, forward=True):
        """gmg_get_gs_schedule: what the setup of the level's Gauss-Seidel smoother built for one direction, on a partitioned level the
        schedule of this rank's own x own block -> dict(nsets, max_set_rows, nlaunches, nwide)"""
        v = [C.c_int64(0) for _ in range(4)]
        abi.check(self.h, self._lib.gmg_get_gs_schedule(self.h, level, 0 if forward else 1, *[C.byref(q) for q in v]))
        return dict(zip(("nsets", "max_set_rows", "nlaunches", "nwide"), (q.value for q in v)))

    def gs_ordering(self, level=0):
        """gmg_get_gs_ordering -> dict(kind, ncolors, order): the visiting order of this rank's own block of the level"""
        L = self.local["levels"][level]
        kind, nc = C.c_int(0), C.c_int64(0)
        order = np.empty(L.n_own, dtype=np.int32)
        abi.check(self.h, self._lib.gmg_get_gs_ordering(self.h, level, C.byref(kind), C.byref(nc), C.c_void_p(order.ctypes.data), order.size))
        return dict(kind=("natural", "multicolor", "given")[kind.value], ncolors=nc.value, order=order)

    def comm_info(self):
        """what the handle communicates through (gmg_get_comm_info): transport, rank, ranks, ncclCommCount, HIP device"""
        v = [C.c_int(0) for _ in range(5)]
        abi.check(self.h, self._lib.gmg_get_comm_info(self.h, *[C.byref(x) for x in v]))
        return dict(transport=("none", "rccl", "host")[v[0].value], rank=v[1].value, nranks=v[2].value, rccl_comm_count=v[3].value,
                    device=v[4].value)

    def halo_info(self, lev=0):
        """what the setup decided for the own | ghost split of partitioned level `lev` (gmg_get_halo_info): boundary rows, send slots,
        ghost entries, the fix-up's form ("none" / "csr" / "sliced" / "sliced+dict") and its dictionary's distinct-value count, whether
        the pack is fused into the fix-up, whether R is split and the same figures for its ghost part"""
        i64 = [C.c_int64(0) for _ in range(5)]
        i32 = [C.c_int(0) for _ in range(6)]
        abi.check(self.h, self._lib.gmg_get_halo_info(self.h, lev, C.byref(i64[0]), C.byref(i64[1]), C.byref(i64[2]), C.byref(i32[0]),
                                                      C.byref(i32[1]), C.byref(i32[2]), C.byref(i32[3]), C.byref(i64[3]), C.byref(i64[4]),
                                                      C.byref(i32[4]), C.byref(i32[5])))
        forms = ("none", "csr", "sliced", "sliced+dict")
        return dict(boundary_rows=int(i64[0].value), send_slots=int(i64[1].value), ghost_entries=int(i64[2].value),
                    fix_form=forms[i32[0].value], dict_values=i32[1].value, pack_fused=bool(i32[2].value), r_split=bool(i32[3].value),
                    r_boundary_rows=int(i64[3].value), r_ghost_entries=int(i64[4].value), r_form=forms[i32[4].value],
                    r_dict_values=i32[5].value)

    def close(self):
        if getattr(self, "h", None):
            self._lib.gmg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------------------------------
# Communication model of a partitioned V-cycle: which levels to replicate, how many ghost layers the others carry
# ---------------------------------------------------------------------------------------------------------------------------
# Measured on MI355X (profiles/r03_rccl_latency.json, tools/rccl_latency.py; RCCL 2.26 self send/recv, 7 messages): one halo
# exchange costs 28-42 us of stream time issued in-stream and 51-63 us with the event hand-off to a second stream; the host needs
# 23-36 us to enqueue it.  A 1-double all-reduce + sqrt: 5-6 us on one rank.  Sweep kernels: 9.0 ns per 1000 rows (row-pattern
# layout, pair sweep: 213 us per sweep on 2.36e7 rows, 16 us on 2.05e6 -- profiles/r04_288_kernel_stats.txt; round 2: 11.3)
# with a floor of 4.4 us + 1.5 us of dependent-launch gap per launch; a whole block of k
# sweeps as ONE launch (<= 5.08e5 rows: sells_smooth_kernel): 2.8 us + 6.0e-6 us per row per sweep (profiles/r02_tuning.md section 6).
MODEL = dict(exchange_us=40.0, exchange_overlapped_us=60.0, link_GBs=50.0, sweep_ns_per_krow=9.0, launch_floor_us=5.9,
             one_launch_rows=507904, one_launch_base_us=2.8, one_launch_us_per_row=6.0e-6, allreduce_us=30.0, allreduce_GBs=50.0,
             # boundary fix-up of an own | ghost sweep (ghost_fix_sell_kernel, dictionary-coded values): 15.4 us for the 2.5e5 boundary rows
             # of a corner rank of 2 x 2 x 2 x 288^3, measured with that rank alone on the GPU (tools/rank_alone.sh; the CSR form took 25.3)
             fixup_us_per_krow=0.062, fixup_floor_us=3.0)


def _pass_us(n_own_cells, depth, niter, m=MODEL, nfaces=3):
    """modelled time of one smoothing pass of `niter` sweeps on a level with n_own_cells^3 owned cells per rank and `depth` ghost
    layers (0 = own | ghost layout with the exchange overlapped with the own x own kernel; nfaces = faces of the rank's box that
    touch a neighbour: their rows are finished by the boundary fix-up after the halo has arrived)"""
    c = n_own_cells
    if depth == 0:
        t_sweep = max(m["launch_floor_us"], c ** 3 * m["sweep_ns_per_krow"] * 1e-6)
        fix = max(m["fixup_floor_us"], nfaces * c * c * 1e-3 * m["fixup_us_per_krow"])
        return niter * (max(t_sweep, m["exchange_overlapped_us"]) + fix)          # + boundary fix-up launch
    rows = (c + 2 * depth) ** 3
    nblk = -(-niter // depth)
    msg_us = depth * c * c * 8.0 / (m["link_GBs"] * 1e3)                            # one face, `depth` layers
    if rows <= m["one_launch_rows"]:
        t_sweeps = nblk * m["one_launch_base_us"] + niter * (m["one_launch_base_us"] + rows * m["one_launch_us_per_row"])
    else:
        t_sweeps = niter * max(m["launch_floor_us"], rows * m["sweep_ns_per_krow"] * 1e-6)
    return t_sweeps + nblk * (m["exchange_us"] + msg_us + 4.0)                      # + scaled-Jacobi launch per block


def plan_partition(cells_per_rank, nlevels, world, niter=10, rep_rows=400000, depth_choices=(0, 1, 2, 3, 5, 6, 10, 11)):
    """(rep_from, depths, table): replicate every level whose GLOBAL size is <= rep_rows dofs (latency-bound: redundant compute beats
    any exchange); give every other level the halo depth that minimises the modelled smoothing-pass time.  The finest level keeps the
    own | ghost layout while its own x own kernel hides the exchange (288^3 cells per GPU: 215 us per sweep against 60 us); below
    ~170^3 cells per rank a sweep is shorter than the exchange and the finest level goes into the overlapping layout as well (depths[0]
    > 0: DistributedGMG(finest_depth=...), separate Krylov operator), charged with its two index passes per V-cycle."""
    grid = pa.rank_grid(world, 3)
    rep_rows = int(os.environ.get("GMG_REP_ROWS", rep_rows))
    rep_from = nlevels - 1
    for l in range(1, nlevels):
        if po.level_sizes(tuple(cells_per_rank * g // 2 ** l for g in grid), 1) <= rep_rows:
            rep_from = l
            break
    depths, table = [0] * nlevels, []
    for l in range(nlevels):
        c = cells_per_rank // 2 ** l
        if l >= rep_from or world == 1:
            table.append(dict(level=l, cells_per_rank=c, layout="replicated" if world > 1 else "single GPU"))
            continue
        nfaces = sum(1 for gk in grid if gk > 1)               # (2 ranks per partitioned direction: one neighbour face each)
        cand = {k: _pass_us(c, k, niter, nfaces=nfaces) for k in depth_choices if k == 0 or (k <= niter + 1 and c >= 2)}
        # consistent!(r) before the restriction (one per V-cycle = half of one per pass) is unnecessary when the LAST block of a pass is
        # shorter than the halo is deep (partition.overlap_hints: depth 3 -> blocks 3,3,3,1; 6 -> 6,4; 11 -> one block of 10)
        for k in cand:
            if k > 0 and k - (niter - min(k, niter) * ((niter - 1) // min(k, niter))) < 1:
                cand[k] += 0.5 * (MODEL["exchange_us"] + 4.0)
        if l == 0:
            # r scattered into / z gathered from the extended-box numbering: two launches of 16 B per owned row per V-cycle = per two passes
            idx_us = max(MODEL["launch_floor_us"], c ** 3 * 16.0 / 4.0e6)
            cand = {k: v + (idx_us if k > 0 else 0.0) for k, v in cand.items()}
        best = min(cand, key=cand.get)
        depths[l] = best
        # the same level on a SUBSET of M ranks (np_per_level of the reference; DistributedGMG(sub_from=..., sub_ranks=M)): each member
        # holds world / M times the rows, and every pass pays one redistribution (latency + n_own doubles over one link) -- reported so
        # that the choice "all ranks" is visible as a number; the planner never picks a subset unless this beats `best`
        subset = {}
        if l >= 1:
            for M in (1, 2, 4):
                if M >= world:
                    continue
                cm = c * (world / M) ** (1.0 / 3.0)
                redist_us = MODEL["exchange_us"] + c ** 3 * 8.0 / (MODEL["link_GBs"] * 1e3)
                subset[str(M)] = round(min(_pass_us(cm, k, niter) for k in depth_choices if k <= niter and (k > 0 or M > 1)) + redist_us, 1)
        table.append(dict(level=l, cells_per_rank=c, layout="own|ghost, exchange overlapped" if best == 0 else f"overlapping, depth {best}",
                          modelled_pass_us={str(k): round(v, 1) for k, v in cand.items()},
                          modelled_pass_us_on_rank_subset=subset,
                          exchanges_per_pass=niter if best == 0 else -(-niter // best)))
    env = os.environ.get("GMG_HALO_DEPTH")
    if env is not None:
        depths = [depths[0]] + [int(env) if l < rep_from else 0 for l in range(1, nlevels)]
    env0 = os.environ.get("GMG_FINEST_DEPTH")
    if env0 is not None and world > 1:
        depths[0] = int(env0)
    return rep_from, depths, table


def run_bench(args, rank, world, local_rank):
    """bench.py --gpus N (N > 1): weak scaling, `cells` cells per direction per GPU."""
    import torch
    import torch.distributed as dist
    nc = (args.cells,) * 3
    transport = os.environ.get("GMG_TRANSPORT", "rccl")
    # STRICT by default: a `--gpus N` line is the product's RCCL path or no line at all (non-zero exit).  The host-staged transport and
    # the in-stream exchange are fallbacks for debugging -- only with --allow-degraded, or in the several-ranks-on-one-GPU test set-up
    # (GMG_SHARE_GPU, which asks for GMG_TRANSPORT=host itself).
    strict = bool(os.environ.get("GMG_BENCH_STRICT_RCCL")) or not (getattr(args, "allow_degraded", False) or os.environ.get("GMG_SHARE_GPU"))
    if strict and transport != "rccl":
        raise SystemExit(f"bench.py --gpus {world}: GMG_TRANSPORT={transport} is not the product's transport (RCCL); pass --allow-degraded to run it anyway")
    group = None
    lengths = tuple(float(v) for v in pa.rank_grid(world, 3))      # cubic cells at every GPU count
    # BASELINE configs[3] (SURVEY 8 size table): 288^3 cells per GPU, 6 levels -> 576,288,144,72,36,18 cells per direction on
    # 2x2x2 GPUs; the GLOBAL coarsest level (dense inverse, replicated) has 17^3 dofs
    nlev = args.levels
    # replicate every level whose GLOBAL size is small (<= 4e5 dofs: at config 4 that is the 72^3 level, 3.6e5 dofs):
    # those levels are latency bound -- a sweep takes 5-7 us, a grouped RCCL send/recv tens of us -- so computing them
    # redundantly on every GPU is cheaper than a halo exchange per sweep
    rep_from, depths, plan_table = plan_partition(args.cells, nlev, world)
    rdev0 = "cpu" if dist.get_backend() == "gloo" else "cuda"

    def all_ok(ok):
        """joint decision: 1 only if every rank succeeded (a per-rank try/except would let ranks diverge into different collectives)"""
        t = torch.tensor([0.0 if ok else 1.0], dtype=torch.float64, device=rdev0)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t.item() == 0.0

    g, err = None, None
    if transport != "host":
        # probe first: a rank that cannot even load librccl would leave the others blocked inside ncclCommInitRank
        probe_ok = True
        try:
            buf = C.create_string_buffer(128)
            probe_ok = abi.load().gmg_comm_unique_id(rccl_path().encode(), buf) == abi.OK
        except Exception as e:
            probe_ok, err = False, e
        if not all_ok(probe_ok):
            if rank == 0:
                print(f"[bench] librccl could not be loaded on at least one rank (rank 0: {err}); falling back to the host-staged transport",
                      flush=True, file=sys.stderr)
            if strict:
                raise RuntimeError("librccl could not be loaded on at least one rank (pass --allow-degraded to fall back to the host-staged transport)")
            transport = "host"
    if transport != "host":
        try:
            g = DistributedGMG(nc, nlev, rank, world, device_id=local_rank, transport="rccl", lengths=lengths, rep_from=rep_from, depth=depths,
                               finest_depth=depths[0])
        except Exception as e:
            err = e
        if not all_ok(g is not None):
            # some rank could not bring the RCCL path up.  Every rank takes this branch (joint decision above): fall back to
            # the host-staged test transport so that the run still shows the distributed algorithm working, and say so loudly
            # -- `degraded` / `transport` in the JSON line; such a number is NOT the product's RCCL path.
            if g is not None:
                g.close()
                g = None
            if rank == 0:
                print(f"[bench] RCCL transport unavailable on at least one rank (rank 0: {err}); falling back to the host-staged transport",
                      flush=True, file=sys.stderr)
            if strict:
                raise RuntimeError(f"RCCL transport unavailable on at least one rank (this rank: {err}); pass --allow-degraded to fall back to the host-staged transport")
            transport = "host"
    if transport == "host":
        group = dist.new_group(backend="gloo") if dist.get_backend() != "gloo" else None
        g = DistributedGMG(nc, nlev, rank, world, device_id=local_rank, transport="host", group=group, lengths=lengths, rep_from=rep_from, depth=depths,
                           finest_depth=depths[0])
    b = g.rhs_lin()
    bd = torch.from_numpy(b).cuda()
    xd = torch.zeros(g.n_own, dtype=torch.float64, device="cuda")
    maxiter, atol, rtol = 20, 1e-14, 1e-6

    def sane():
        """One untimed solve; every rank agrees on whether it converged to the analytic solution."""
        xd.zero_(); torch.cuda.synchronize()
        lg = g.cg_solve(bd, xd, maxiter, atol, rtol)
        bad = float(np.max(np.abs(xd.cpu().numpy() - g.exact_own()))) > 1e-3 or lg.num_iters >= maxiter
        t = torch.tensor([1.0 if bad else 0.0], dtype=torch.float64, device=rdev0)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t.item() == 0.0

    overlap_note = "halo overlapped with the own x own mat-vec" if transport == "rccl" else "no overlap"
    degraded = transport != "rccl"
    if not sane() and transport == "rccl":
        # safety net: the overlapped exchange (comm stream + events) cannot be exercised on the 1-GPU
        # development boxes; if it ever misbehaves fall back to in-stream exchanges and say so
        if strict:
            raise RuntimeError("overlapped halo exchange gave a wrong solution (pass --allow-degraded to retry with in-stream exchanges)")
        if rank == 0:
            print("[bench] overlapped halo exchange gave a wrong solution; retrying with GMG_OVERLAP=0", flush=True, file=sys.stderr)
        os.environ["GMG_OVERLAP"] = "0"
        g.close()
        g = DistributedGMG(nc, nlev, rank, world, device_id=local_rank, transport="rccl", lengths=lengths, rep_from=rep_from, depth=depths,
                           finest_depth=depths[0])
        overlap_note = "in-stream halo exchange (overlap disabled after a failed self-check)"
        degraded = True
        if not sane():
            raise RuntimeError("distributed solve does not reproduce the analytic solution")

    rdev = "cpu" if dist.get_backend() == "gloo" else "cuda"

    def timed(gh, steps, warmup):
        """`steps` timed solves of handle gh (barrier + synchronize on both sides, max over ranks)"""
        def step():
            xd.zero_()
            torch.cuda.synchronize()
            return gh.cg_solve(bd, xd, maxiter, atol, rtol)
        for _ in range(warmup):
            lg = step()
        # HIP events on every stride-th finest sweep of the timed solves: each sample costs the stream ~11 us, so keep them rare
        # (largest of 61 / 31 / 13 / 7 that leaves >= 8 samples; GMG_PROF_STRIDE overrides)
        stride = int(os.environ["GMG_PROF_STRIDE"]) if os.environ.get("GMG_PROF_STRIDE") else next((s for s in (61, 31, 13, 7) if steps * 60 // s >= 8), 7)
        abi.check(gh.h, gh._lib.gmg_set_option(gh.h, b"prof_stride", float(stride)))
        gh.profile(0, True)
        ex0, ar0 = gh.comm_stats()
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            lg = step()
        torch.cuda.synchronize()
        dist.barrier()
        dt = time.perf_counter() - t0
        ex1, ar1 = gh.comm_stats()
        st = gh.kernel_stats()
        gh.profile(0, False)
        tmax = torch.tensor([dt], dtype=torch.float64, device=rdev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        e = torch.tensor([float(np.max(np.abs(xd.cpu().numpy() - gh.exact_own())))], dtype=torch.float64, device=rdev)
        dist.all_reduce(e, op=dist.ReduceOp.MAX)
        avg_ms = st["total_ms"] / max(st["launches"], 1)
        return dict(dt=float(tmax.item()), steps=steps, iters=int(lg.num_iters), err=float(e.item()), st=st, avg_ms=avg_ms,
                    exchanges_per_solve=(ex1 - ex0) / steps, allreduces_per_solve=(ar1 - ar0) / steps)

    n = g.n_global
    D = timed(g, args.steps, args.warmup)
    st, avg_ms = D["st"], D["avg_ms"]
    achieved = st["alg_bytes"] / (avg_ms * 1e-3) / 1e9 if st["launches"] else None
    layout_GBs = st["layout_bytes"] / (avg_ms * 1e-3) / 1e9 if st["launches"] else None
    setup_s, asm_s, rep_lvl = g.t_setup, g.t_assembly, int(g.local["rep_from"])
    grid_s, cg_s = "x".join(map(str, g.grid)), "x".join(map(str, g.cells_global))
    # who really took part: what RCCL reports for the communicator, and the device every rank sits on
    ci = g.comm_info()
    props = torch.cuda.get_device_properties(torch.cuda.current_device())
    mine = dict(rank=rank, local_rank=local_rank, device=ci["device"], rccl_comm_count=ci["rccl_comm_count"], name=props.name,
                uuid=str(getattr(props, "uuid", "")), pci_bus_id=int(getattr(props, "pci_bus_id", -1)))
    everyone = [None] * world
    dist.all_gather_object(everyone, mine)
    sig = g.sweep_signature(0)
    if strict and not (transport == "rccl" and ci["rccl_comm_count"] == world and all(e["rccl_comm_count"] == world for e in everyone)):
        raise RuntimeError(f"RCCL communicator reports {[e['rccl_comm_count'] for e in everyone]} ranks, expected {world} on every rank")
    out = {
        "metric": "DoFs/sec, CG+GMG V-cycle on 3D Poisson Q1",
        "value": n * D["steps"] / D["dt"], "unit": "DoFs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": D["dt"] / D["steps"] * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic", "headline_leg": "default",
        "legs": LEGS_NOTE,
        "rccl_ranks": ci["rccl_comm_count"] if transport == "rccl" else 0,
        "devices": everyone,
        "config": {
            "workload": f"BASELINE configs[3] shape: 3D Poisson Q1, {args.cells}^3 cells per GPU on a {grid_s} GPU grid "
                        f"(global {cg_s} cells on (0,{'x'.join(str(int(v)) for v in lengths)}): cubic cells), {nlev}-level GMG V-cycle, "
                        f"Richardson(Jacobi,10,2/3), CG rtol={rtol:g}, rhs = u=x1+x2 Dirichlet lift; row partition + "
                        f"halo exchange + scalar all-reduce ({transport}; {overlap_note})",
            "dofs": n, "dofs_per_gpu": g.n_own, "levels": nlev, "cg_iterations": D["iters"],
            "transport": transport, "degraded": bool(degraded), "replicated_from_level": rep_lvl, "max_abs_error_vs_exact": D["err"],
            "halo_depths": depths, "partition_plan": plan_table, "communication_model": MODEL,
            "transfer_exchanges_skipped": [[bool(a), bool(b)] for a, b in getattr(g, "overlap_hints", [])],   # per level: consistent!(r) before R, consistent!(dxh) before r -= A dxh
            "halo_exchanges_per_solve": D["exchanges_per_solve"], "allreduces_per_solve": D["allreduces_per_solve"],
            "setup_s": setup_s, "assembly_s": asm_s,
        },
        # default leg: the local operators are constant-coefficient here, so the own x own kernel runs the row-pattern layout; its
        # honest figure is bytes-actually-moved / time (layout_bytes) -- the 12 B/nnz model describes the generic leg (`roofline`)
        "roofline_compressed": {"leg": "default", "leg_value": n * D["steps"] / D["dt"], "leg_ms_per_step": D["dt"] / D["steps"] * 1e3,
                                "pairs_with": "value / ms_per_step",
                                "bound": "hbm", "kernel": "fused Richardson-Jacobi sweep, own x own part (rank 0, finest level)", "sweep_signature": sig,
                                "achieved": layout_GBs, "peak": 8000.0, "unit": "GB/s",
                                "frac": (layout_GBs / 8000.0) if layout_GBs else None, "traffic": None,
                                "bytes_model": "gmg_kernel_stats.layout_bytes (matrix stream as stored + row-wise vectors, each once)",
                                "bytes_per_launch": st["layout_bytes"], "model_12B_per_nnz_GBs": achieved,
                                "avg_launch_ms": avg_ms, "launches_timed": st["launches"]},
    }
    # ---- generic leg: the same partitioned problem on the plain 12 B/nnz stream (what SURVEY 8(d)'s byte model describes) ----
    if not getattr(args, "no_generic", False):
        g.close()
        gg = None
        try:
            gg = DistributedGMG(nc, nlev, rank, world, device_id=local_rank, transport=transport, group=group, lengths=lengths, rep_from=rep_from,
                                depth=depths, options=GENERIC_OPTIONS, finest_depth=depths[0])
        except Exception as e:
            err = e
        if all_ok(gg is not None):
            G = timed(gg, max(2, args.steps // 3), 1)
            stg = G["st"]
            ach = stg["alg_bytes"] / (G["avg_ms"] * 1e-3) / 1e9 if stg["launches"] else None
            out["value_generic"] = n * G["steps"] / G["dt"]
            out["ms_per_step_generic"] = G["dt"] / G["steps"] * 1e3
            out["config"]["cg_iterations_generic"] = G["iters"]
            out["roofline"] = {"leg": "generic", "leg_value": out["value_generic"], "leg_ms_per_step": out["ms_per_step_generic"],
                               "pairs_with": "value_generic / ms_per_step_generic",
                               "bound": "hbm", "kernel": "sell_kernel<EPI_SWEEP,ONEG> own x own part (rank 0, finest level), 12 B/nnz (col,val) stream",
                               "sweep_signature": gg.sweep_signature(0),
                               "achieved": ach, "peak": 8000.0, "unit": "GB/s", "frac": (ach / 8000.0) if ach else None, "traffic": None,
                               "bytes_model": "SURVEY 8(d): B_sweep = 12 Z + 68 N on this rank's rows", "bytes_per_launch": stg["alg_bytes"],
                               "avg_launch_ms": G["avg_ms"], "launches_timed": stg["launches"]}
            gg.close()
        else:
            if gg is not None:
                gg.close()
            out["roofline"] = {"leg": "generic", "error": f"generic leg could not be set up on every rank ({err})"}
    else:
        g.close()
        out["roofline"] = {"leg": "generic", "skipped": "--no-generic"}
    return out


# the generic (12 B/nnz) leg: every structure-exploiting storage layout off -- per-handle options (gmg_set_option), not environment
GENERIC_OPTIONS = {"vdict": 0, "idx16": 0, "pattern": 0, "opattern": 0}
LEGS_NOTE = ("same key <-> leg mapping at every --gpus N: default leg (the product as shipped: gmg_setup picks the storage layout) = `value`, "
             "`ms_per_step`, `roofline_compressed`; generic leg (every structure-exploiting layout off: the 12 B/nnz (col,val) stream SURVEY 8(d)'s "
             "byte model describes) = `value_generic`, `ms_per_step_generic`, `roofline`.  N = 1 runs BASELINE configs[1] (128^3) and carries the "
             "per-GPU problem of the N > 1 runs on one GPU as `weak_anchor_value` / `weak_scaling_ref`; N > 1 runs 288^3 cells per GPU: hold "
             "value / N against weak_anchor_value, never against the N = 1 `value`.")


class DistributedBlockSolver:
    """Distributed counterpart of solvers.BlockNumericalSetup for a 2x2 block system whose blocks live on two levels of the
    partitioned hierarchy (the multi-rank shape of test/Applications/mpi/StokesGMG.jl: BlockTriangularSolver on BlockPMatrix /
    BlockPVector, BlockTriangularSolvers.jl:216-242).  `gmg` is a set-up DistributedGMG (the solver of block 0); block 1 is
    solved by CGSolver(JacobiLinearSolver()) on `M11`.  All matrices are this rank's LOCAL rows with [own | ghost] columns."""

    def __init__(self, gmg: DistributedGMG, A01, A10, M11, lev0, lev1, A11=None, coeffs=((1.0, 1.0), (0.0, 1.0)), half="upper",
                 cg=(20, 1e-14, 1e-6)):
        lib = gmg._lib
        self._lib, self.gmg = lib, gmg
        sizes = np.array([lev0.n_own, lev1.n_own], dtype=np.int64)
        self.sizes, self.n = sizes, int(sizes.sum())
        h = C.c_void_p()
        kind = {"diagonal": abi.BLOCK_DIAGONAL, "lower": abi.BLOCK_LOWER, "upper": abi.BLOCK_UPPER}[half]
        dev = 0
        try:
            import torch
            dev = torch.cuda.current_device()
        except Exception:
            pass
        abi.check_block(None, lib.gmg_block_create(C.byref(h), 2, C.c_void_p(sizes.ctypes.data), kind, dev))
        self.h = h
        self._keep = []
        if gmg.world > 1:
            if gmg.transport == "rccl_loopback":
                path = rccl_path().encode()
                uid = C.create_string_buffer(128)
                abi.check(None, lib.gmg_comm_unique_id(path, uid))
                abi.check_block(h, lib.gmg_block_comm_init_rccl(h, path, bytes(uid.raw), 0, 1))
                abi.check_block(h, lib.gmg_block_comm_set_loopback(h, gmg.world))
            elif gmg.transport == "host_loopback":
                hb = gmg._host
                abi.check_block(h, lib.gmg_block_comm_init_host(h, 0, 1, C.cast(hb.exchange_cb, C.c_void_p), C.cast(hb.allreduce_cb, C.c_void_p), None))
                abi.check_block(h, lib.gmg_block_comm_set_loopback(h, gmg.world))
            elif gmg.transport == "rccl":
                import torch.distributed as dist
                path = rccl_path().encode()
                uid = C.create_string_buffer(128)
                if gmg.rank == 0:
                    abi.check(None, lib.gmg_comm_unique_id(path, uid))
                blob = [bytes(uid.raw) if gmg.rank == 0 else None]
                dist.broadcast_object_list(blob, src=0)
                abi.check_block(h, lib.gmg_block_comm_init_rccl(h, path, blob[0], gmg.rank, gmg.world))
            else:
                hb = gmg._host
                abi.check_block(h, lib.gmg_block_comm_init_host(h, gmg.rank, gmg.world, C.cast(hb.exchange_cb, C.c_void_p),
                                                                C.cast(hb.allreduce_cb, C.c_void_p), None))
            for j, L in enumerate((lev0, lev1)):
                nbr = np.ascontiguousarray(L.nbr_rank, dtype=np.int32)
                sp, si, rp = (np.ascontiguousarray(a, dtype=np.int64) for a in (L.snd_ptr, L.snd_idx, L.rcv_ptr))
                self._keep += [nbr, sp, si, rp]
                abi.check_block(h, lib.gmg_block_set_partition(h, j, L.n_own, L.n_ghost, nbr.size, C.c_void_p(nbr.ctypes.data),
                                                               C.c_void_p(sp.ctypes.data), C.c_void_p(si.ctypes.data), C.c_void_p(rp.ctypes.data)))

        def setb(fn, i, j, M):
            idx64 = M.idx.astype(np.int64)
            abi.check_block(h, fn(h, i, j, M.shape[0], M.shape[1], M.nnz, C.c_void_p(M.ptr.ctypes.data), C.c_void_p(idx64.ctypes.data),
                                  C.c_void_p(M.val.ctypes.data), abi.CSR, 0, 8))
        setb(lib.gmg_block_set_system_block, 0, 0, lev0.A)
        setb(lib.gmg_block_set_system_block, 0, 1, A01)
        setb(lib.gmg_block_set_system_block, 1, 0, A10)
        if A11 is not None:
            setb(lib.gmg_block_set_system_block, 1, 1, A11)
        for i in range(2):
            for j in range(2):
                if i != j:
                    abi.check_block(h, lib.gmg_block_set_coeff(h, i, j, float(coeffs[i][j])))
        abi.check_block(h, lib.gmg_block_set_diag_gmg(h, 0, gmg.h))
        abi.check_block(h, lib.gmg_block_set_diag_solver(h, 1, abi.BLOCK_CG_JACOBI, cg[0], cg[1], cg[2]))
        idx64 = M11.idx.astype(np.int64)
        abi.check_block(h, lib.gmg_block_set_diag_matrix(h, 1, M11.shape[0], M11.nnz, C.c_void_p(M11.ptr.ctypes.data), C.c_void_p(idx64.ctypes.data),
                                                         C.c_void_p(M11.val.ctypes.data), abi.CSR, 0, 8))
        abi.check_block(h, lib.gmg_block_setup(h))

    def precond_apply(self, b, x):
        pb, ms, _k1 = _vec(b, self.n)
        px, ms2, _k2 = _vec(x, self.n, writable=True)
        abi.check_block(self.h, self._lib.gmg_block_precond_apply(self.h, pb, px, ms))
        return x

    def fgmres_solve(self, b, x, m=20, maxiter=100, atol=1e-10, rtol=1e-12):
        log = ConvergenceLog("FGMRES", maxiter, atol, rtol)
        pb, ms, _k1 = _vec(b, self.n)
        px, ms2, _k2 = _vec(x, self.n, writable=True)
        res = abi.Result()
        hist = np.zeros(maxiter + 1)
        abi.check_block(self.h, self._lib.gmg_block_fgmres_solve(self.h, pb, px, ms, m, 0, 1, maxiter, atol, rtol, 1, C.byref(res),
                                                                 C.c_void_p(hist.ctypes.data), hist.size))
        log._fill(res, hist)
        return log

    def gmres_solve(self, b, x, m=20, maxiter=100, atol=1e-10, rtol=1e-12, restart=False, m_add=1, side="right"):
        """GMRESSolver(m; Pr=this block preconditioner) (side="right") or with it as Pl ("left") on the partitioned block system
        (GMRESSolvers.jl:132-210)"""
        log = ConvergenceLog("GMRES", maxiter, atol, rtol)
        pb, ms, _k1 = _vec(b, self.n)
        px, ms2, _k2 = _vec(x, self.n, writable=True)
        assert side in ("right", "left")
        res = abi.Result()
        hist = np.zeros(maxiter + 1)
        abi.check_block(self.h, self._lib.gmg_block_gmres_solve(self.h, pb, px, ms, m, int(restart), m_add, maxiter, atol, rtol,
                                                                int(side == "right"), int(side == "left"), C.byref(res),
                                                                C.c_void_p(hist.ctypes.data), hist.size))
        log._fill(res, hist)
        return log

    def minres_solve(self, b, x, maxiter=100, atol=1e-10, rtol=1e-12):
        """MINRESSolver(;Pl=this block preconditioner) on the partitioned block system (MINRESSolvers.jl:75-148)"""
        log = ConvergenceLog("MINRES", maxiter, atol, rtol)
        pb, ms, _k1 = _vec(b, self.n)
        px, ms2, _k2 = _vec(x, self.n, writable=True)
        res = abi.Result()
        hist = np.zeros(maxiter + 1)
        abi.check_block(self.h, self._lib.gmg_block_minres_solve(self.h, pb, px, ms, maxiter, atol, rtol, 1, C.byref(res),
                                                                 C.c_void_p(hist.ctypes.data), hist.size))
        log._fill(res, hist)
        return log

    def close(self):
        if getattr(self, "h", None):
            self._lib.gmg_block_destroy(self.h)
            self.h = None
