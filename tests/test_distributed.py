"""Multi-process tests of the row-partitioned path: world_size 2/4/8 over gloo.

CPU (not gpu): partition + exchange plans + distributed algorithm emulated in numpy on the
local operators, against the serial oracle.  GPU: the same through libgmgamd with the
host-staged transport (all ranks share the one GPU of the test box)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import thread_ranks  # noqa: E402


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


_PORT_BUSY = ("EADDRINUSE", "address already in use", "Address already in use")


def _run_with_fresh_port(build_cmd, attempts=4, **kw):
    """subprocess.run(build_cmd(port), ...) -- again with another port when the rendezvous lost the race for it (the port _free_port()
    found free can be taken by the time rank 0 listens on it: the GPU boxes are shared, and one such collision under `pytest -x` would end
    the whole run: it did once in 5 suite runs of round 6)."""
    out = None
    for _ in range(attempts):
        out = subprocess.run(build_cmd(_free_port()), **kw)
        if out.returncode == 0 or not any(t in (out.stdout or "") + (out.stderr or "") for t in _PORT_BUSY):
            break
    return out


def _launch(mode, world, cells, nlev, tmp_path, transport="host", timeout=600, rep_from=0, extra_env=None, _attempt=0):
    out = os.path.join(str(tmp_path), f"verdict_{mode}_{world}.json")
    port = _free_port()
    procs = []
    # a GPU partition wider than GPU_PROCS ranks runs as threads of ONE process: the shared GPU machines allow few GPU processes
    threaded = mode.startswith("gpu") and world > thread_ranks.GPU_PROCS
    assert not (threaded and (extra_env or {}).get("GMG_HOST_ASYNC")), "the asynchronous host schedule needs a process per rank"
    for r in range(1 if threaded else world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0", **(extra_env or {}), **({"GMG_TEST_THREAD_RANKS": "1"} if threaded else {}))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_worker.py"), mode,
                                       "x".join(map(str, cells)), str(nlev), out, transport, str(rep_from)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    import time as _time
    logs = []
    t_end = _time.time() + timeout
    # a rank that dies leaves the others blocked in a collective: stop waiting as soon as one has failed
    while _time.time() < t_end and any(p.poll() is None for p in procs) and not any(p.poll() not in (None, 0) for p in procs):
        _time.sleep(0.2)
    if any(p.poll() not in (None, 0) for p in procs):
        _time.sleep(2.0)
    for p in procs:
        if p.poll() is None:
            p.kill()
    for r, p in enumerate(procs):
        o, _ = p.communicate()
        logs.append(f"---- rank {r} (rc {p.returncode}) ----\n" + o.decode(errors="replace")[-3000:])
    if any(p.returncode != 0 for p in procs) and _attempt < 3 and any(t in "\n".join(logs) for t in _PORT_BUSY):
        return _launch(mode, world, cells, nlev, tmp_path, transport, timeout, rep_from, extra_env, _attempt + 1)   # lost the race for the port
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    v = json.load(open(out))
    if os.path.exists(out + ".x.npy"):
        v["x"] = np.load(out + ".x.npy")                     # gathered solution (global numbering)
    return v


def _check(v):
    assert v["iters"] == v["iters_oracle"] and v["iters_all_equal"], v
    assert v["rel_err"] < 1e-10 and v["hist_dev"] < 1e-8, v
    assert v["l2_error_sq"] < 1e-8, v


@pytest.mark.parametrize("world,cells,nlev,rep", [(2, (8, 8, 8), 2, 0), (4, (8, 8), 2, 0), (8, (4, 4, 4), 2, 0), (8, (8, 8, 8), 3, 1)])
def test_partitioned_cg_gmg_numpy_gloo(world, cells, nlev, rep, tmp_path):
    """rep = first replicated level (0: only the coarsest)."""
    _check(_launch("numpy", world, cells, nlev, tmp_path, rep_from=rep))


@pytest.mark.parametrize("world,cells,nlev,rep,depth", [(2, (16, 16, 16), 3, 2, 2), (8, (8, 8, 8), 3, 2, 2), (4, (16, 16), 4, 3, 3),
                                                          (2, (16, 16, 16), 3, 2, 10)])
def test_overlapping_layout_numpy_gloo(world, cells, nlev, rep, depth, tmp_path):
    """Partitioned levels >= 1 in the overlapping layout (gmg_set_partition_overlap): `depth` ghost layers, one exchange per
    `depth` sweeps, ghost rows recomputed redundantly.  Same iteration count and history as the serial oracle, and fewer halo
    exchanges than the own | ghost schedule by the expected amount."""
    v0 = _launch("numpy", world, cells, nlev, tmp_path, rep_from=rep)
    v = _launch("numpy", world, cells, nlev, tmp_path, rep_from=rep, extra_env={"GMG_TEST_DEPTH": str(depth)})
    _check(v0); _check(v)
    nov = rep - 1                                            # levels 1 .. rep-1 are in the overlapping layout
    per_pass0, per_pass = 10, -(-10 // depth)
    saved = v["iters"] * nov * 2 * (per_pass0 - per_pass)    # two smoothing passes per level and V-cycle, one V-cycle per CG iteration
    saved += v["iters"] * v["hint_skips"]                    # + the transfer exchanges the geometry makes unnecessary (partition.overlap_hints)
    assert v0["exchanges"] - v["exchanges"] == saved, (v0["exchanges"], v["exchanges"], saved)


def test_overlapping_layout_operators_match_global(po, pkg):
    """Local operators of the overlapping layout: owned rows of A / P / R reproduce the global mat-vecs, ghost rows of R are empty,
    both sides of every exchange enumerate the same global ids, every ghost is received exactly once."""
    from gridapsolvers_jl_amd import partition as pa
    for nc, nlev, nranks, rep, depth in [((16, 16, 16), 3, 8, 2, 2), ((16, 16, 16), 3, 2, 2, 3), ((32, 32), 4, 4, 3, 2)]:
        grid = pa.rank_grid(nranks, len(nc))
        Hg = po.build_hierarchy(nc, nlev, 1)
        locs = [pa.build_local_hierarchy(nc, nlev, grid, r, 1, None, rep, depth) for r in range(nranks)]
        assert any(L.overlap for L in locs[0]["levels"]) and not locs[0]["levels"][0].overlap
        for l in range(nlev):
            N = Hg["mats"][l].shape[0]
            x = np.random.default_rng(l).uniform(-1, 1, N)
            yg = Hg["mats"][l].matvec(x)
            owned = np.zeros(N, dtype=int)

            def loc_vec(L, v):
                return v[L.local_gid] if L.overlap else (v if L.replicated else np.concatenate([v[L.own_gid], v[L.ghost_gid]]))
            for r in range(nranks):
                L = locs[r]["levels"][l]
                if L.replicated:
                    continue
                owned[L.own_gid] += 1
                y = L.A.matvec(loc_vec(L, x))
                assert np.abs((y[L.own_idx] if L.overlap else y) - yg[L.own_gid]).max() < 1e-13
                if L.overlap:
                    assert L.A.shape == (L.n_local, L.n_local) and np.array_equal(np.sort(np.concatenate([L.own_idx, L.rcv_idx])), np.arange(L.n_local))
                    for k, q in enumerate(L.nbr_rank):
                        Lq = locs[q]["levels"][l]
                        kk = list(Lq.nbr_rank).index(r)
                        assert np.array_equal(L.local_gid[L.snd_idx[L.snd_ptr[k]:L.snd_ptr[k + 1]]], Lq.local_gid[Lq.rcv_idx[Lq.rcv_ptr[kk]:Lq.rcv_ptr[kk + 1]]])
                if l < nlev - 1:
                    Lc = locs[r]["levels"][l + 1]
                    xc = np.random.default_rng(9).uniform(-1, 1, Hg["mats"][l + 1].shape[0])
                    yp, ypg = L.P.matvec(loc_vec(Lc, xc)), Hg["prolongations"][l].matvec(xc)
                    assert np.abs((yp[L.own_idx] if L.overlap else yp) - ypg[L.own_gid]).max() < 1e-14
                    yr, yrg = L.R.matvec(loc_vec(L, x)), Hg["restrictions"][l].matvec(x)
                    if Lc.overlap:
                        assert np.abs(yr[Lc.own_idx] - yrg[Lc.own_gid]).max() < 1e-13
                        assert np.abs(np.delete(yr, Lc.own_idx)).max(initial=0.0) == 0.0
                    elif Lc.replicated:
                        assert np.abs(yr - yrg[locs[r]["rep_gid"]]).max() < 1e-13
                    else:
                        assert np.abs(yr - yrg[Lc.own_gid]).max() < 1e-13
            if not locs[0]["levels"][l].replicated:
                assert (owned == 1).all()


def test_partition_operators_match_global(po, pkg):
    """Local operators / exchange plans reproduce the global mat-vecs on every level (no processes)."""
    from gridapsolvers_jl_amd import partition as pa
    for nc, nlev, nranks in [((8, 8, 8), 2, 8), ((16, 8, 8), 2, 2), ((16, 16), 3, 4)]:
        grid = pa.rank_grid(nranks, len(nc))
        Hg = po.build_hierarchy(nc, nlev, 1)
        locs = [pa.build_local_hierarchy(nc, nlev, grid, r, 1, None, nlev) for r in range(nranks)]   # nothing replicated
        for l in range(nlev):
            N = Hg["mats"][l].shape[0]
            x = np.random.default_rng(l).uniform(-1, 1, N)
            yg = Hg["mats"][l].matvec(x)
            assert sum(loc["levels"][l].n_own for loc in locs) == N
            for r in range(nranks):
                L = locs[r]["levels"][l]
                xl = np.concatenate([x[L.own_gid], x[L.ghost_gid]])
                assert np.abs(L.A.matvec(xl) - yg[L.own_gid]).max() < 1e-13
                if l < nlev - 1:
                    Lc = locs[r]["levels"][l + 1]
                    xc = np.random.default_rng(9).uniform(-1, 1, Hg["mats"][l + 1].shape[0])
                    xcl = np.concatenate([xc[Lc.own_gid], xc[Lc.ghost_gid]])
                    assert np.abs(L.P.matvec(xcl) - Hg["prolongations"][l].matvec(xc)[L.own_gid]).max() < 1e-14
                    assert np.abs(L.R.matvec(xl) - Hg["restrictions"][l].matvec(x)[Lc.own_gid]).max() < 1e-13
                for k, q in enumerate(L.nbr_rank):
                    Lq = locs[q]["levels"][l]
                    kk = list(Lq.nbr_rank).index(r)
                    sent = L.own_gid[L.snd_idx[L.snd_ptr[k]:L.snd_ptr[k + 1]]]
                    assert np.array_equal(sent, Lq.ghost_gid[Lq.rcv_ptr[kk]:Lq.rcv_ptr[kk + 1]])


@pytest.mark.parametrize("world,cells,nlev,rep", [(2, (4, 4, 4), 2, 0), (4, (8, 8), 3, 0), (8, (4, 4, 4), 2, 0), (2, (8, 8), 3, 1)])
def test_partitioned_patch_smoother_numpy_gloo(world, cells, nlev, rep, tmp_path):
    """Q2 + the distributed vertex-star patch smoother (consistent!(b), owned patches, assemble!(x), consistent!(x);
    PatchSolvers.jl:227-236,251-258) emulated in numpy over gloo: CG+GMG iteration count identical to the serial oracle."""
    v = _launch("numpy", world, cells, nlev, tmp_path, rep_from=rep, extra_env={"GMG_TEST_ORDER": "2", "GMG_TEST_SMOOTHER": "patch"})
    _check(v)


@pytest.mark.parametrize("world,cells,nlev,rep,order,smoother,depth,saved_per_pass",
                         [(2, (8, 8), 3, 2, 2, "patch", 2, 6), (2, (8, 8), 3, 2, 2, "patch", 1, 4), (4, (8, 8), 3, 2, 2, "jacobi", 2, 5),
                          (2, (8, 8, 8), 3, 2, 2, "patch", 2, 6), (2, (8, 8), 3, 2, 1, "patch", 2, 6)])
def test_overlapping_layout_q2_and_patch_smoothers_numpy_gloo(world, cells, nlev, rep, order, smoother, depth, saved_per_pass, tmp_path):
    """The overlapping layout beyond Q1 + Jacobi (round 4), emulated in numpy over gloo: Q2 levels with Richardson(Jacobi) (a sweep
    consumes `order` node layers) and Richardson(PatchSolver) on vertex stars (3 order - 2 layers per sweep; every star inside the
    extended box is solved locally: no assemble!, no consistent!(dx) inside a block).  CG+GMG reproduces the serial oracle
    (iterations identical, history <= 1e-8, solution <= 1e-10) and the exchanges per solve drop by exactly
    iterations x 2 passes x saved_per_pass on the one overlapping level (patch, niter = 4: 2 x 4 exchanges per pass become ceil(4 / depth);
    Jacobi, niter = 10: 10 become ceil(10 / depth))."""
    env = {"GMG_TEST_ORDER": str(order), "GMG_TEST_SMOOTHER": smoother}
    v0 = _launch("numpy", world, cells, nlev, tmp_path, rep_from=rep, extra_env=env)
    v = _launch("numpy", world, cells, nlev, tmp_path, rep_from=rep, extra_env=dict(env, GMG_TEST_DEPTH=str(depth)))
    _check(v0)
    _check(v)
    assert v["iters"] == v0["iters"]
    assert v0["exchanges"] - v["exchanges"] == v0["iters"] * (2 * saved_per_pass + v["hint_skips"]), (v0["exchanges"], v["exchanges"], v["hint_skips"])


def test_overlap_vertex_star_patches_cover_the_owned_dofs(po, pkg):
    """partition._OverlapGeom.vertex_star_patches: every vertex star of the serial table that touches an owned dof is in the local
    table, with the same dofs (through the local -> global map) in the same relative order"""
    from gridapsolvers_jl_amd import partition as pa
    for cg, grid, order, depth in (((16, 8), (2, 1), 2, 1), ((8, 8, 8), (2, 2, 1), 2, 1), ((16, 16), (2, 2), 1, 2)):
        pp, pd = po.vertex_star_patches(cg, order)
        serial = [tuple(pd[pp[p]:pp[p + 1]]) for p in range(pp.size - 1) if pp[p + 1] > pp[p]]
        for rank in range(int(np.prod(grid))):
            og = pa._OverlapGeom(tuple(cg) + (1,) * (3 - len(cg)), tuple(grid) + (1,) * (3 - len(grid)), rank, len(cg), depth, order, 3 * order - 2)
            lp, ld = og.vertex_star_patches()
            local = [tuple(og.gid[ld[lp[p]:lp[p + 1]]]) for p in range(lp.size - 1)]
            own = set(og.own_gid.tolist())
            need = [s for s in serial if own & set(s)]
            assert [s for s in serial if s in set(local)] == local          # a sub-sequence of the serial table, same order
            assert all(s in set(local) for s in need)


def test_partition_operators_match_global_q2(po, pkg):
    """order 2: halo of 3 nodes (R = P^T reaches the quarter points of both adjacent coarse cells); owned vertex-star patches of
    all ranks = the serial patch set, each patch exactly once, local numbering consistent with the ghost layout."""
    from gridapsolvers_jl_amd import partition as pa
    for nc, nlev, nranks in [((8, 8, 8), 2, 8), ((8, 4, 4), 2, 2), ((16, 16), 3, 4)]:
        grid = pa.rank_grid(nranks, len(nc))
        Hg = po.build_hierarchy(nc, nlev, 2)
        locs = [pa.build_local_hierarchy(nc, nlev, grid, r, 2, None, nlev) for r in range(nranks)]
        for l in range(nlev):
            N = Hg["mats"][l].shape[0]
            x = np.random.default_rng(l).uniform(-1, 1, N)
            yg = Hg["mats"][l].matvec(x)
            for r in range(nranks):
                L = locs[r]["levels"][l]
                xl = np.concatenate([x[L.own_gid], x[L.ghost_gid]])
                assert np.abs(L.A.matvec(xl) - yg[L.own_gid]).max() < 1e-12
                if l < nlev - 1:
                    Lc = locs[r]["levels"][l + 1]
                    xc = np.random.default_rng(9).uniform(-1, 1, Hg["mats"][l + 1].shape[0])
                    xcl = np.concatenate([xc[Lc.own_gid], xc[Lc.ghost_gid]])
                    assert np.abs(L.P.matvec(xcl) - Hg["prolongations"][l].matvec(xc)[L.own_gid]).max() < 1e-13
                    assert np.abs(L.R.matvec(xl) - Hg["restrictions"][l].matvec(x)[Lc.own_gid]).max() < 1e-12
        for l in range(nlev - 1):
            pp, pd = po.vertex_star_patches(Hg["ncells"][l], 2)
            serial = sorted(tuple(pd[pp[p]:pp[p + 1]]) for p in range(pp.size - 1) if pp[p + 1] > pp[p])
            got = []
            for r in range(nranks):
                lp, ll, lg = pa.local_vertex_star_patches(Hg["ncells"][l], 2, grid, r)
                L = locs[r]["levels"][l]
                assert (np.concatenate([L.own_gid, L.ghost_gid])[ll] == lg).all()
                got += [tuple(lg[lp[p]:lp[p + 1]]) for p in range(lp.size - 1) if lp[p + 1] > lp[p]]
            assert sorted(got) == serial


@pytest.mark.gpu
@pytest.mark.parametrize("world,cells,nlev,rep", [(2, (4, 4, 4), 2, 0), (8, (4, 4, 4), 2, 0), (4, (8, 8), 3, 1)])
def test_partitioned_patch_smoother_on_gpu_host_transport(world, cells, nlev, rep, tmp_path):
    """the same through libgmgamd: reverse halo (assemble!) + ghost-reaching patches with caller-assembled patch matrices."""
    v = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep,
                extra_env={"GMG_TEST_ORDER": "2", "GMG_TEST_SMOOTHER": "patch"})
    _check(v)


@pytest.mark.gpu
@pytest.mark.parametrize("world,cells,nlev,rep", [(2, (16, 16, 16), 3, 0), (8, (8, 8, 8), 2, 0), (4, (16, 16), 3, 0), (2, (16, 16, 16), 4, 2), (8, (8, 8, 8), 3, 1)])
def test_partitioned_cg_gmg_on_gpu_host_transport(world, cells, nlev, rep, tmp_path):
    v = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep)
    _check(v)
    assert v["fgmres_iters"] <= v["iters"] + 1 and v["fgmres_vs_cg"] < 1e-5
    if world == 2:
        # the kernels the big partitioned levels of the bench take (two rows per lane: mat-vecs on the own x own part, prolongation +
        # correction), forced onto these small levels: same bits
        w = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep, extra_env={"GMG_PAT_R2MV_MIN": "1"})
        _check(w)
        assert w["iters"] == v["iters"]
        np.testing.assert_array_equal(w["x"], v["x"])
        # round 5: the z-walk form of the sweep and of the mat-vecs (what the 288^3-per-GPU finest level of BASELINE configs[3] runs), forced
        # onto these small partitioned levels -- own x own part of an own | ghost level, n_own rows x (n_own + n_ghost) columns: same bits
        z = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep,
                    extra_env={"GMG_PAT_R2MV_MIN": "1", "GMG_PAT_ZWALK": "2", "GMG_PAT_ZWALK_T": "3"})
        _check(z)
        assert z["iters"] == v["iters"]
        np.testing.assert_array_equal(z["x"], v["x"])
    # the boundary fix-up of the own | ghost levels in its two forms (slices of 64 boundary rows, column-major: the default; one thread
    # walking a CSR row): same products in the same order
    c = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep, extra_env={"GMG_HALO_FIX_SELL": "0"})
    _check(c)
    assert c["iters"] == v["iters"] and c["x_sha"] == v["x_sha"]
    np.testing.assert_array_equal(c["x"], v["x"])


@pytest.mark.gpu
@pytest.mark.parametrize("world,cells,nlev,rep", [(2, (16, 16, 16), 4, 3), (8, (8, 8, 8), 3, 2), (4, (32, 32), 4, 3)])
def test_overlapping_layout_on_gpu_host_transport(world, cells, nlev, rep, tmp_path):
    """The real library with levels >= 1 in the overlapping layout (several ranks on one GPU, host transport): iteration counts
    and histories of the serial oracle; halo exchanges per solve drop by the expected amount; the sweeps of a block run as one
    launch (sells_smooth_kernel between two exchanges) or launch by launch give IDENTICAL bits; different depths agree to rounding
    (owned rows of the level operators are summed in the same order whatever the depth, but the restriction's layout -- and with
    it the summation tree of the CSR-stream kernel -- depends on how many empty ghost rows it carries)."""
    env = {"GMG_PERSIST_SHARED": "1"}
    v0 = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep)
    vs = {d: _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep, extra_env=dict(env, GMG_TEST_DEPTH=str(d))) for d in (1, 2, 5)}
    vl = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep, extra_env={"GMG_TEST_DEPTH": "5", "GMG_PERSIST": "0"})
    _check(v0)
    for v in list(vs.values()) + [vl]:
        _check(v)
        assert v["iters"] == v0["iters"]
    assert np.array_equal(vs[5]["x"], vl["x"])
    for d in (1, 2):
        assert np.linalg.norm(vs[d]["x"] - vs[5]["x"]) <= 1e-13 * np.linalg.norm(vs[5]["x"])
    assert np.linalg.norm(vs[5]["x"] - v0["x"]) <= 1e-12 * np.linalg.norm(v0["x"])
    nov = rep - 1
    assert vs[1]["exchanges"] == v0["exchanges"] - v0["iters"] * vs[1]["hint_skips"]   # depth 1: the same count per pass, whole rows in one kernel
    for d in (2, 5):
        assert v0["exchanges"] - vs[d]["exchanges"] == v0["iters"] * (nov * 2 * (10 - -(-10 // d)) + vs[d]["hint_skips"]), (v0["exchanges"], vs[d]["exchanges"])


@pytest.mark.gpu
@pytest.mark.parametrize("world,cells,nlev,rep", [(2, (16, 16, 16), 4, 3), (8, (8, 8, 8), 3, 2), (4, (32, 32), 4, 3)])
def test_streamed_operators_on_partitioned_levels(world, cells, nlev, rep, tmp_path):
    """gmg_set_operator_rows with several ranks: every level matrix but the coarsest and the transfers between single-GPU-like levels
    (overlapping layout, replicated) arrive in blocks of 97 rows and are kept in row-pattern form only; on the own | ghost finest
    level the library splits each block into the own x own part (stream) and the ghost columns (boundary fix-up CSR) -- same iteration
    count as the run that hands every operator over whole, solutions equal to rounding (whole transfers of this size go through the
    CSR-stream kernel, whose lanes-per-row tree sums a row in another order than the pattern kernels' left-to-right)."""
    env = {"GMG_PERSIST_SHARED": "1", "GMG_TEST_DEPTH": "2"}
    v = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep, extra_env=env)
    w = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep, extra_env=dict(env, GMG_TEST_STREAM_ROWS="97"))
    _check(w)
    assert len(w["streamed_levels"]) >= 2 and 0 in w["streamed_levels"] and v["streamed_levels"] == []   # the own | ghost finest level too
    assert w["iters"] == v["iters"]
    assert np.max(np.abs(w["x"] - v["x"])) <= 1e-13 * np.max(np.abs(v["x"]))


@pytest.mark.gpu
@pytest.mark.parametrize("world,cells,nlev,rep,order,smoother,depth,saved_per_pass",
                         [(2, (8, 8, 8), 3, 2, 2, "patch", 2, 6), (4, (8, 8), 3, 2, 2, "patch", 4, 7), (2, (8, 8, 8), 3, 2, 2, "jacobi", 5, 8),
                          (8, (8, 8, 8), 3, 2, 2, "patch", 1, 4)])
def test_overlapping_layout_q2_and_patch_smoothers_on_gpu_host_transport(world, cells, nlev, rep, order, smoother, depth, saved_per_pass, tmp_path):
    """The real library with a Q2 level in the overlapping layout under Richardson(Jacobi) and Richardson(PatchSolver) (several ranks
    on one GPU, host transport): iteration counts and histories of the serial oracle, the exchanges per solve drop by exactly
    iterations x 2 x saved_per_pass, and the result agrees with the own | ghost run to rounding."""
    env = {"GMG_TEST_ORDER": str(order), "GMG_TEST_SMOOTHER": smoother, "GMG_PERSIST_SHARED": "1"}
    v0 = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep, extra_env=env)
    v = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep, extra_env=dict(env, GMG_TEST_DEPTH=str(depth)))
    _check(v0)
    _check(v)
    assert v["iters"] == v0["iters"]
    assert v0["exchanges"] - v["exchanges"] == v0["iters"] * (2 * saved_per_pass + v["hint_skips"]), (v0["exchanges"], v["exchanges"], v["hint_skips"])
    assert np.linalg.norm(v["x"] - v0["x"]) <= 1e-11 * np.linalg.norm(v0["x"])
    if world == 2:
        # round 5: the wide-row operators of these levels in the z-walk form (sellw_zwalk_kernel, forced with pat_zwalk = 2): same bits
        z = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep,
                    extra_env=dict(env, GMG_TEST_DEPTH=str(depth), GMG_PAT_ZWALK="2", GMG_PAT_ZWALK_T="2", GMG_PAT_CODED_MIN_ROWS="0"))
        w = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep,
                    extra_env=dict(env, GMG_TEST_DEPTH=str(depth), GMG_PAT_ZWALK="0", GMG_PAT_CODED_MIN_ROWS="0"))
        _check(z)
        assert z["iters"] == w["iters"]
        np.testing.assert_array_equal(z["x"], w["x"])


@pytest.mark.gpu
def test_partitioned_operators_big_enough_for_the_eager_pattern_scan(tmp_path):
    """Local matrices of >= 20 000 rows: on one GPU such structured CSR inputs are kept in row-pattern form only.  A distributed
    setup splits own / ghost columns on the CSR, so the scan must stay off once the communicator exists (the ABI requires
    gmg_comm_init_* before rectangular local matrices are accepted at all)."""
    v = _launch("gpu", 2, (32, 32, 32), 3, tmp_path, transport="host", rep_from=2)
    _check(v)


@pytest.mark.gpu
@pytest.mark.parametrize("world,cells,nlev,rep", [(2, (16, 16, 16), 3, 0), (4, (8, 8, 8), 3, 1)])
def test_overlapped_schedule_with_async_host_transport(world, cells, nlev, rep, tmp_path):
    """The two-stream / two-event schedule of the RCCL path (halo on comm_stream while the own x own kernel
    runs, boundary rows afterwards) driven by the host transport through hipLaunchHostFunc: real concurrency
    between the exchange and the kernel, on one GPU.  One process per rank (the callbacks run on HIP's host-function
    thread), so at most thread_ranks.GPU_PROCS ranks: a 2 x 2 x 1 grid, face and edge neighbours."""
    v = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep, extra_env={"GMG_HOST_ASYNC": "1"})
    _check(v)


@pytest.mark.gpu
@pytest.mark.parametrize("world,cells,nlev", [(2, (16, 16, 16), 3), (4, (16, 16), 3), (8, (8, 8, 8), 3)])
def test_distributed_block_triangular_fgmres_on_gpu_host_transport(world, cells, nlev, tmp_path):
    """Multi-rank block preconditioner (BlockTriangularSolvers.jl:216-242 on BlockPVector / BlockPMatrix, the solver shape of
    test/Applications/mpi/StokesGMG.jl): distributed GMG(maxiter=4) on block 0, CG-Jacobi on block 1, upper triangular, outer
    FGMRES(20) -- one application and the whole solve against the serial oracle; halo exchanges of the off-diagonal blocks'
    operands, all-reduced dots, distributed GMG handle borrowed by the block handle."""
    v = _launch("gpu_block", world, cells, nlev, tmp_path, transport="host")
    assert v["iters"] == v["iters_oracle"] and v["iters_all_equal"], v
    # ~50 non-restarted FGMRES steps: the Arnoldi residual estimate amplifies the (different) summation order of the
    # all-reduced dots; held to 1e-4 of the initial residual, the solution itself to 1e-7
    assert v["precond_rel_err"] < 1e-9 and v["rel_err"] < 1e-7 and v["hist_dev"] < 1e-4, v
    assert v["true_residual"] < 1e-7, v                                      # StokesGMG.jl:166


@pytest.mark.gpu
def test_rccl_binding_selftest_single_rank(pkg):
    """The dlopen'ed RCCL entry points (ncclGetUniqueId/CommInitRank/AllReduce/Send/Recv/Group*) work on
    real hardware: 1-rank communicator, all-reduce and a grouped self send/recv on the handle's stream."""
    import ctypes as C
    from gridapsolvers_jl_amd import abi, multigpu
    lib = abi.load()
    h = C.c_void_p()
    abi.check(None, lib.gmg_create(C.byref(h), 2, 0))
    path = multigpu.rccl_path().encode()
    uid = C.create_string_buffer(128)
    abi.check(None, lib.gmg_comm_unique_id(path, uid))
    abi.check(h, lib.gmg_comm_init_rccl(h, path, bytes(uid.raw), 0, 1))
    out = (C.c_double * 2)()
    abi.check(h, lib.gmg_comm_selftest(h, out))
    assert out[0] == 1.5 and out[1] == 42.0
    # the latency probe behind DESIGN.md section 5's communication model (tools/rccl_latency.py): sane, positive stream times
    lat = (C.c_double * 6)()
    abi.check(h, lib.gmg_comm_latency_probe(h, 7, 1024, 20, lat))
    assert all(0.0 < lat[i] < 5e4 for i in (0, 2, 4, 5)), list(lat)
    lib.gmg_destroy(h)


@pytest.mark.gpu
@pytest.mark.parametrize("finest", [None, 0])
def test_bench_multi_rank_path_with_overlapping_levels(finest, tmp_path):
    """`bench.py --gpus 2` with the planner forced to keep level 1 partitioned in the overlapping layout (depth 5): the N > 1 line
    carries both legs, the partition plan and the per-solve exchange counts.  At 32^3 cells per rank the planner puts the FINEST level
    into the overlapping layout too (depth 11: one block of ten sweeps per pass and a residual that is still exact where the restriction reads it; separate Krylov operator); GMG_FINEST_DEPTH=0
    keeps it own | ghost as at BASELINE config 4's size."""
    import subprocess
    env = dict(os.environ, GMG_SHARE_GPU="1", GMG_TRANSPORT="host", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1",
               GMG_BENCH_DETAILS=str(tmp_path / "legs.json"),
               GMG_REP_ROWS="3000", GMG_HALO_DEPTH="5", **({} if finest is None else {"GMG_FINEST_DEPTH": str(finest)}))
    root = os.path.dirname(HERE)
    out = _run_with_fresh_port(lambda port: [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                                             "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--cells", "32", "--levels", "4",
                                             "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][0]
    assert len(line) <= 4096 and json.loads(line)["details"] == str(tmp_path / "legs.json")
    d = json.load(open(tmp_path / "legs.json"))           # everything the run measured; the printed line is its <= 4 KB extract
    assert d["n_gpus"] == 2 and d["headline_leg"] == "default" and d["roofline"]["leg"] == "default" and d["roofline_generic"]["leg"] == "generic"
    assert d["config"]["halo_depths"][:3] == [11 if finest is None else finest, 5, 0] and d["config"]["replicated_from_level"] == 2
    assert d["config"]["cg_iterations"] == d["config"]["cg_iterations_generic"] <= 4 and d["config"]["max_abs_error_vs_exact"] < 1e-4
    assert d["value_generic"] > 0 and d["config"]["halo_exchanges_per_solve"] > 0


@pytest.mark.gpu
def test_bench_multi_rank_path_runs_end_to_end_on_one_gpu(tmp_path):
    """`bench.py --gpus 2` as the driver launches it (torch.distributed.run, one rank per process), both ranks sharing the single
    GPU of the test box over the host-staged transport: the JSON contract of the multi-rank line and the joint self-check."""
    import subprocess
    env = dict(os.environ, GMG_SHARE_GPU="1", GMG_TRANSPORT="host", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1",
               GMG_BENCH_DETAILS=str(tmp_path / "legs.json"))
    root = os.path.dirname(HERE)
    out = _run_with_fresh_port(lambda port: [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                                             "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--cells", "32", "--levels", "3",
                                             "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-1500:]
    # the printed line: <= 4 KB, ONE leg (value, ms_per_step and roofline all describe the default leg), the driver's contract keys
    assert len(lines[0]) <= 4096
    ln = json.loads(lines[0])
    assert set(ln) >= {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                       "dtype", "data", "config", "roofline"} and ln["roofline"]["leg"].startswith("default")
    assert ln["n_gpus"] == 2 and ln["steps"] == 2 and ln["unit"] == "DoFs/s" and ln["scaling"] == "weak" and ln["value"] > 0
    assert ln["config"]["transport"] == "host" and ln["config"]["degraded"] is True and "workload" in ln["config"]
    assert ln["roofline"]["frac"] is None or ln["roofline"]["frac"] <= 1.0
    d = json.load(open(tmp_path / "legs.json"))           # everything else: the details file the line names
    assert ln["details"] == str(tmp_path / "legs.json") and d["value"] == ln["value"] and d["ms_per_step"] == ln["ms_per_step"]
    assert d["config"]["cg_iterations"] <= 4 and d["config"]["max_abs_error_vs_exact"] < 1e-4
    # the same shape as the N = 1 record: default leg = `roofline`, generic leg = `roofline_generic`; who took part; the anchor
    assert d["roofline_generic"]["leg"] == "generic" and d["roofline"]["leg"] == "default"
    assert d["rccl_ranks"] == 0 and len(d["devices"]) == 2 and {x["rank"] for x in d["devices"]} == {0, 1}
    assert d["weak_anchor_value"] > 0 and d["weak_scaling_ref"]["cg_iterations"] == d["config"]["cg_iterations"]


@pytest.mark.gpu
@pytest.mark.parametrize("world,n,nlev", [(2, 8, 2), (4, 16, 3), (2, 16, 3), (8, 16, 3)])
def test_distributed_real_stokes_on_gpu_host_transport(world, n, nlev, tmp_path):
    """BASELINE configs[4] in its multi-rank form (test/Applications/mpi/StokesGMG.jl:5-12): the lid-driven-cavity Q2 / P1disc
    system partitioned by cell boxes over `world` ranks (all on the one GPU of the test box, host transport) -- vector-valued
    velocity hierarchy with owned vertex-star patch smoothers and the DISTRIBUTED patch-corrected prolongation, CG-Jacobi
    pressure block, upper block-triangular preconditioner, FGMRES(20): iteration counts equal the serial oracle's, solution
    <= 1e-6, true residual < 1e-7 (StokesGMG.jl:166), discretely divergence-free."""
    v = _launch("gpu_stokes", world, (n, n), nlev, tmp_path, transport="host")
    assert v["gmg_iters"] == v["gmg_iters_oracle"] and v["gmg_rel_err"] < 1e-8, v
    assert v["iters"] == v["iters_oracle"] and v["iters_all_equal"], v
    assert v["rel_err"] < 1e-6 and v["hist_dev"] < 1e-6, v
    assert v["true_residual"] < 1e-7 and v["div_residual"] < 1e-7 and v["umax"] > 0.3, v
    assert v["ghosts"][0] > 0 and v["ghosts"][1] > 0


def test_generic_partitioner_reproduces_the_stokes_operators(po, pkg):
    """dpartition.py on the Q2 / P1disc Stokes blocks and the velocity hierarchy: local operators reproduce the global mat-vecs,
    every dof has exactly one owner, both sides of every exchange agree, owned patches cover the serial patch set exactly once."""
    from gridapsolvers_jl_amd import stokes as st, dpartition as dp, partition as pa
    n, nlev, nranks = 8, 2, 4
    grid = pa.rank_grid(nranks, 2)
    sysd, Hv = st.stokes_system(n), st.velocity_hierarchy(n, nlev)
    V = [dp.Space(f"v{l}", st.velocity_owner(Hv["ncells"][l], grid), nranks) for l in range(nlev)]
    Pq = dp.Space("p", st.pressure_owner(n, grid), nranks)
    A = sysd["A"]
    ops = [(A[0][0].to_scipy(), V[0], V[0]), (A[0][1].to_scipy(), V[0], Pq), (A[1][0].to_scipy(), Pq, V[0]),
           (Hv["restrictions"][0].to_scipy(), V[1], V[0]), (Hv["graddiv"][0].to_scipy(), V[0], V[0])]
    pp, pd = Hv["star_patches"][0]
    powner = st.patch_owner(pp, pd, V[0].owner)
    dp.partition_spaces(V + [Pq], ops, [(pp, pd, V[0], powner)])
    rng = np.random.default_rng(0)
    for M, rs, cs in ops:
        x = rng.uniform(-1, 1, cs.n)
        y = M @ x
        for r in range(nranks):
            Ml = dp.local_operator(M, rs, cs, r)
            assert np.abs(Ml.matvec(x[cs.local_gid(r)]) - y[rs.own[r]]).max() < 1e-11
    for S_ in V + [Pq]:
        assert sum(S_.n_own(r) for r in range(nranks)) == S_.n
        for r in range(nranks):
            pl = S_.plan[r]
            for k, q in enumerate(pl["nbr_rank"]):
                plq = S_.plan[q]
                kk = list(plq["nbr_rank"]).index(r)
                sent = S_.own[r][pl["snd_idx"][pl["snd_ptr"][k]:pl["snd_ptr"][k + 1]]]
                assert np.array_equal(sent, S_.ghost[q][plq["rcv_ptr"][kk]:plq["rcv_ptr"][kk + 1]])
    got = []
    for r in range(nranks):
        ptr, loc, glob, blocks = dp.local_patches(pp, pd, V[0], powner, r, Hv["mats"][0].to_scipy())
        assert np.array_equal(V[0].local_gid(r)[loc], glob) and blocks.size == int(((ptr[1:] - ptr[:-1]) ** 2).sum())
        got += [tuple(glob[ptr[p]:ptr[p + 1]]) for p in range(ptr.size - 1) if ptr[p + 1] > ptr[p]]
    assert sorted(got) == sorted(tuple(pd[pp[p]:pp[p + 1]]) for p in range(pp.size - 1) if pp[p + 1] > pp[p])


@pytest.mark.parametrize("world,n", [(2, 8), (4, 8), (8, 16)])
def test_partitioned_stokes_system_numpy_gloo(world, n, tmp_path):
    """The partitioned Q2 / P1disc block system over gloo (CPU): consistent! of both spaces through the generic partitioner's
    exchange plans, then every rank's rows -- the gathered product equals K x; and assemble! (reverse halo add) on the velocity
    space equals a global scatter-add.  Ranks without pressure ghosts still send (discontinuous pressure)."""
    v = _launch("numpy_stokes", world, (n, n), 2, tmp_path)
    assert v["matvec_err"] < 1e-13 and v["assemble_err"] == 0.0, v
    assert v["ghosts"][0] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("world,cells,nlev,rep,stream", [(2, (16, 16, 16), 4, 3, 97), (4, (32, 32), 4, 3, 97), (2, (16, 16, 16), 4, 3, 0)])
def test_value_refresh_on_a_streamed_own_ghost_level(world, cells, nlev, rep, stream, tmp_path):
    """numerical_setup! (gmg_update_values on every level + gmg_setup) on a partitioned hierarchy whose own | ghost finest level was
    STREAMED (gmg_set_operator_rows: own x own part in the row-pattern stream, ghost columns in the boundary fix-up CSR): the caller's
    whole-row value array is routed into both parts.  All values doubled and b doubled: the second solve reproduces the first --
    same iteration count on every rank, x to rounding (bitwise in practice: scaling by 2 is exact).  Before round 5 the ghost-column
    values kept their old numbers and the refreshed operator was silently wrong.  stream = 0: the same through whole CSR levels."""
    env = {"GMG_PERSIST_SHARED": "1", "GMG_TEST_DEPTH": "2", "GMG_TEST_REFRESH": "1"}
    if stream:
        env["GMG_TEST_STREAM_ROWS"] = str(stream)
    v = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep, extra_env=env)
    _check(v)
    if stream:
        assert 0 in v["streamed_levels"]
    assert v["refresh_iters"] == [v["iters"]] * world, v
    assert v["refresh_dev"] <= 1e-13, v


FINEST_CASES = [(2, (16, 16, 16), 3, 2, 2, 2), (8, (8, 8, 8), 3, 2, 2, 5), (4, (16, 16), 4, 3, 3, 2), (2, (16, 16, 16), 3, 1, 0, 3)]


@pytest.mark.parametrize("world,cells,nlev,rep,depth,fdepth", FINEST_CASES)
def test_finest_level_in_the_overlapping_layout_numpy_gloo(world, cells, nlev, rep, depth, fdepth, tmp_path):
    """The FINEST level in the overlapping layout too (`fdepth` ghost layers): the Krylov solver keeps the own | ghost vectors and
    operator (one exchange per mat-vec), the preconditioner's level 0 smooths in the extended-box numbering with one exchange per
    `fdepth` sweeps.  Iteration count and history of the serial oracle; exchanges saved on level 0 exactly
    iterations x 2 passes x (10 - ceil(10 / fdepth))."""
    v0 = _launch("numpy", world, cells, nlev, tmp_path, rep_from=rep, extra_env={"GMG_TEST_DEPTH": str(depth)})
    v = _launch("numpy", world, cells, nlev, tmp_path, rep_from=rep, extra_env={"GMG_TEST_DEPTH": str(depth), "GMG_TEST_FINEST_DEPTH": str(fdepth)})
    _check(v0); _check(v)
    saved = v["iters"] * 2 * (10 - (-(-10 // fdepth))) + v["iters"] * (v["hint_skips"] - v0["hint_skips"])
    assert v0["exchanges"] - v["exchanges"] == saved, (v0["exchanges"], v["exchanges"], saved)
    assert np.abs(v["x"] - v0["x"]).max() <= 1e-12 * np.abs(v0["x"]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("world,cells,nlev,rep,depth,fdepth", FINEST_CASES)
def test_finest_level_in_the_overlapping_layout_on_gpu_host_transport(world, cells, nlev, rep, depth, fdepth, tmp_path):
    """The real library (several ranks on one GPU, host transport) with the finest level in the overlapping layout and the Krylov
    operator handed over separately (GMG_LEVEL_KRYLOV + gmg_set_krylov_map): CG and FGMRES reproduce the serial oracle's iteration
    count and history, the exchanges per solve drop by exactly iterations x 2 x (10 - ceil(10 / fdepth)), the solution agrees with
    the own | ghost finest level to rounding, and one-launch passes == per-sweep launches bitwise."""
    env = {"GMG_PERSIST_SHARED": "1", "GMG_TEST_DEPTH": str(depth)}
    v0 = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep, extra_env=env)
    v = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep, extra_env=dict(env, GMG_TEST_FINEST_DEPTH=str(fdepth)))
    vl = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep, extra_env=dict(env, GMG_TEST_FINEST_DEPTH=str(fdepth), GMG_PERSIST="0"))
    _check(v0); _check(v); _check(vl)
    assert v["iters"] == v0["iters"] and v["fgmres_iters"] == v0["fgmres_iters"] and v["fgmres_vs_cg"] < 1e-6
    assert v0["exchanges"] - v["exchanges"] == v0["iters"] * (2 * (10 - -(-10 // fdepth)) + v["hint_skips"] - v0["hint_skips"]), (v0["exchanges"], v["exchanges"])
    assert np.linalg.norm(v["x"] - v0["x"]) <= 1e-12 * np.linalg.norm(v0["x"])
    np.testing.assert_array_equal(v["x"], vl["x"])


@pytest.mark.gpu
def test_finest_overlapping_level_with_q2_patch_smoother_on_gpu_host_transport(tmp_path):
    """Q2 + Richardson(PatchSolver) with the finest level in the overlapping layout (depth 2 = 8 node layers): serial oracle's
    iterations; 2 passes x (4 sweeps x 2 forward exchanges - 2 block exchanges) saved per iteration on level 0."""
    env = {"GMG_TEST_ORDER": "2", "GMG_TEST_SMOOTHER": "patch", "GMG_PERSIST_SHARED": "1"}
    v0 = _launch("gpu", 2, (8, 8, 8), 3, tmp_path, transport="host", rep_from=1, extra_env=env)
    v = _launch("gpu", 2, (8, 8, 8), 3, tmp_path, transport="host", rep_from=1, extra_env=dict(env, GMG_TEST_FINEST_DEPTH="2"))
    _check(v0); _check(v)
    assert v["iters"] == v0["iters"]
    assert v0["exchanges"] - v["exchanges"] == v0["iters"] * (2 * 6 + v["hint_skips"]), (v0["exchanges"], v["exchanges"], v["hint_skips"])
    assert np.linalg.norm(v["x"] - v0["x"]) <= 1e-11 * np.linalg.norm(v0["x"])


def test_overlap_space_of_the_vector_valued_stokes_velocity(po, pkg):
    """dpartition.OverlapSpace on the vector-valued Q2 velocity levels: owned rows of the square local operators reproduce the global
    mat-vec (and every row at least 2 nodes inside the local box), the exchange plans of all ranks fit together (what r sends to q
    is what q expects from r, in the same order), every ghost is received exactly once, the local patch lists are the global patches
    that fit in the box, and the sliced transfers reproduce P on owned fine rows / R on owned coarse rows."""
    import importlib
    st = importlib.import_module(pkg.__name__ + ".stokes")
    dp = importlib.import_module(pkg.__name__ + ".dpartition")
    pa = importlib.import_module(pkg.__name__ + ".partition")
    n, nlev, nranks, depth = 16, 3, 4, 1
    grid = pa.rank_grid(nranks, 2)
    Hv = st.velocity_hierarchy(n, nlev)
    cells = Hv["ncells"]

    def coords(c):
        k = np.arange((2 * c - 1) ** 2)
        return np.repeat(np.stack([k % (2 * c - 1) + 1, k // (2 * c - 1) + 1], axis=1), 2, axis=0)
    S = [dp.OverlapSpace(f"v{l}", st.velocity_owner(cells[l], grid), coords(cells[l]), nranks, 4 * depth) for l in range(2)]
    rng = np.random.default_rng(3)
    for l, Sp in enumerate(S):
        A = Hv["mats"][l].to_scipy().tocsr()
        x = rng.uniform(-1, 1, Sp.n)
        y = A @ x
        X = coords(cells[l])
        assert sum(Sp.n_own(r) for r in range(nranks)) == Sp.n
        for r in range(nranks):
            e = Sp.ext[r]
            Al = Sp.square(A, r)
            yl = Al.matvec(x[e])
            assert np.abs(yl[Sp.own_idx(r)] - y[Sp.own[r]]).max() < 1e-11
            lo, hi = X[e].min(axis=0), X[e].max(axis=0)
            nmax = 2 * cells[l] - 1
            inner = (((X[e] - lo >= 2) | (X[e] <= 2)) & ((hi - X[e] >= 2) | (X[e] >= nmax - 1))).all(axis=1)
            assert inner.sum() > Sp.n_own(r) and np.abs(yl[inner] - y[e][inner]).max() < 1e-11
            # exchange emulation: owners' values into my ghosts
            v = np.where(Sp.is_own[r], x[e], np.nan)
            pl = Sp.plan[r]
            for k, q in enumerate(pl["nbr_rank"]):
                plq = Sp.plan[q]
                kk = list(plq["nbr_rank"]).index(r)
                sent = Sp.ext[q][plq["snd_idx"][plq["snd_ptr"][kk]:plq["snd_ptr"][kk + 1]]]          # global ids q sends to r
                want = e[pl["rcv_idx"][pl["rcv_ptr"][k]:pl["rcv_ptr"][k + 1]]]
                assert np.array_equal(sent, want)
                v[pl["rcv_idx"][pl["rcv_ptr"][k]:pl["rcv_ptr"][k + 1]]] = x[sent]
            assert np.array_equal(v, x[e])
            pp, pd = Hv["star_patches"][l]
            ptr, loc = Sp.patches(pp, pd, r)
            glob = {tuple(pd[pp[p]:pp[p + 1]]) for p in range(pp.size - 1)}
            assert ptr.size - 1 > 0 and all(tuple(e[loc[ptr[p]:ptr[p + 1]]]) in glob for p in range(ptr.size - 1))
    P, R = Hv["prolongations"][0].to_scipy().tocsr(), Hv["restrictions"][0].to_scipy().tocsr()
    xc, xf = rng.uniform(-1, 1, S[1].n), rng.uniform(-1, 1, S[0].n)
    for r in range(nranks):
        Pl = dp.sliced_operator(P, S[0].ext[r], S[1].g2l[r], ncols=S[1].n_local(r))
        assert np.abs(Pl.matvec(xc[S[1].ext[r]])[S[0].own_idx(r)] - (P @ xc)[S[0].own[r]]).max() < 1e-12
        Rl = dp.sliced_operator(R, S[1].ext[r], S[0].g2l[r], keep_row=S[1].is_own[r], ncols=S[0].n_local(r), strict_rows=S[1].is_own[r])
        yr = Rl.matvec(xf[S[0].ext[r]])
        assert np.abs(yr[S[1].own_idx(r)] - (R @ xf)[S[1].own[r]]).max() < 1e-12 and not yr[~S[1].is_own[r]].any()


@pytest.mark.gpu
@pytest.mark.parametrize("world,n,nlev,depth", [(4, 16, 3, 1), (2, 32, 4, 2), (4, 64, 4, 2)])      # ((8, 16, 3, 1) passes too: 49 s of process start-up, left out of the suite)
def test_distributed_real_stokes_with_overlapping_velocity_levels(world, n, nlev, depth, tmp_path):
    """Round 5: the partitioned vector-valued velocity levels >= 1 of the distributed Stokes solve in the OVERLAPPING layout
    (dpartition.OverlapSpace; patch smoother AND patch-corrected prolongation with blocks from the local matrix, no assemble!):
    the same iteration counts as the serial oracle for the velocity GMG alone and for the whole FGMRES solve, the same solution as
    the own | ghost run to rounding, fewer halo exchanges."""
    v0 = _launch("gpu_stokes", world, (n, n), nlev, tmp_path, transport="host")
    v = _launch("gpu_stokes", world, (n, n), nlev, tmp_path, transport="host", extra_env={"GMG_TEST_DEPTH": str(depth)})
    for w in (v0, v):
        assert w["gmg_iters"] == w["gmg_iters_oracle"] and w["gmg_rel_err"] < 1e-8, w
        assert w["iters"] == w["iters_oracle"] and w["iters_all_equal"], w
        assert w["rel_err"] < 1e-6 and w["hist_dev"] < 1e-6, w
        assert w["true_residual"] < 1e-7 and w["div_residual"] < 1e-7, w
    assert v["overlap_levels"] == list(range(1, nlev - 1)) and v0["overlap_levels"] == []
    assert v["exchanges"] < v0["exchanges"], (v["exchanges"], v0["exchanges"])


# (4, (8, 8), 3, 2, 1, 2, 0) is test/LinearSolvers/mpi/GMGTests.jl:6-7's np_per_level = [(2,2),(2,1),(1,1)]: level 0 on 2 x 2 ranks, level 1
# on 2 x 1, the coarsest on "one" (here: replicated -- every rank computes it, which is what one rank + a broadcast would deliver)
SUBSET_CASES = [(4, (8, 8, 8), 3, 2, 1, 2, 0), (4, (8, 8), 3, 2, 1, 2, 0), (8, (8, 8, 8), 3, 2, 1, 4, 2), (4, (16, 16), 4, 3, 1, 2, 0),
                (4, (16, 16), 4, 3, 2, 1, 0), (8, (8, 8, 8), 3, 2, 1, 2, 0)]


@pytest.mark.parametrize("world,cells,nlev,rep,sub_from,sub_ranks,depth", SUBSET_CASES)
def test_levels_on_a_rank_subset_numpy_gloo(world, cells, nlev, rep, sub_from, sub_ranks, depth, tmp_path):
    """np_per_level / redistribute! (ModelHierarchies.jl:80-148, GridTransferOperators.jl:447-532): the partitioned levels
    sub_from .. rep-1 on the first `sub_ranks` ranks only.  Level sub_from exists in the glued partition of all ranks and in the
    subset's; the restricted residual and the correction cross with one redistribution each per V-cycle (2 per CG iteration), the
    other ranks shadow the all-reduce of the replicated boundary.  Iteration count, history and solution of the serial oracle."""
    env = {"GMG_TEST_SUB_FROM": str(sub_from), "GMG_TEST_SUB_RANKS": str(sub_ranks), "GMG_TEST_DEPTH": str(depth)}
    v = _launch("numpy", world, cells, nlev, tmp_path, rep_from=rep, extra_env=env)
    _check(v)
    assert v["redistributions"] == 2 * v["iters"], v


@pytest.mark.gpu
@pytest.mark.parametrize("world,cells,nlev,rep,sub_from,sub_ranks,depth", SUBSET_CASES[1:4])
def test_levels_on_a_rank_subset_on_gpu_host_transport(world, cells, nlev, rep, sub_from, sub_ranks, depth, tmp_path):
    """The same through the library (gmg_set_redistribution; several ranks on one GPU, host transport): CG and FGMRES with the serial
    oracle's iteration counts, the solution of the all-rank layout to rounding."""
    env = {"GMG_PERSIST_SHARED": "1", "GMG_TEST_DEPTH": str(depth)}
    v0 = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep, extra_env=env)
    v = _launch("gpu", world, cells, nlev, tmp_path, transport="host", rep_from=rep,
                extra_env=dict(env, GMG_TEST_SUB_FROM=str(sub_from), GMG_TEST_SUB_RANKS=str(sub_ranks)))
    _check(v0); _check(v)
    assert v["iters"] == v0["iters"] and v["fgmres_iters"] == v0["fgmres_iters"] and v["fgmres_vs_cg"] < 1e-6
    assert np.linalg.norm(v["x"] - v0["x"]) <= 1e-12 * np.linalg.norm(v0["x"])


@pytest.mark.gpu
@pytest.mark.parametrize("cycle", ["w_cycle", "f_cycle"])
def test_rank_subset_levels_under_w_and_f_cycles(cycle, tmp_path):
    """W and F cycles visit the subset levels and the replicated boundary below them more than once per cycle: the ranks outside the
    subset must shadow exactly that recursion (`shadow_cycle`), or the all-reduces of the replicated boundary stop matching.  Two
    subset levels (4 ranks -> 2), iteration counts of the serial oracle with the same cycle, the all-rank layout's solution."""
    env = {"GMG_PERSIST_SHARED": "1", "GMG_TEST_CYCLE": cycle}
    v0 = _launch("gpu", 4, (16, 16), 4, tmp_path, transport="host", rep_from=3, extra_env=env)
    v = _launch("gpu", 4, (16, 16), 4, tmp_path, transport="host", rep_from=3, extra_env=dict(env, GMG_TEST_SUB_FROM="1", GMG_TEST_SUB_RANKS="2"))
    _check(v0); _check(v)
    assert v["iters"] == v0["iters"] and np.linalg.norm(v["x"] - v0["x"]) <= 1e-12 * np.linalg.norm(v0["x"])


def test_planner_and_overlap_hints_rules(pkg):
    """multigpu.plan_partition: at BASELINE config 4's size the finest level stays own | ghost (its kernel hides the exchange), levels 1 / 2
    take the depths whose last smoothing block leaves the residual exact where the restriction reads it (6 -> blocks 6,4; 11 -> one
    block of 10), small finest levels go into the overlapping layout, and no rank subset beats the all-rank layouts.
    partition.overlap_hints: the rule behind gmg_set_partition_overlap_hints."""
    import importlib
    mg = importlib.import_module(pkg.__name__ + ".multigpu")
    pa = importlib.import_module(pkg.__name__ + ".partition")
    rep, depths, table = mg.plan_partition(288, 6, 8)
    assert rep == 3 and depths == [0, 6, 11, 0, 0, 0]
    for row in table[1:3]:
        best = min(row["modelled_pass_us"].values())
        assert all(v > best for v in row["modelled_pass_us_on_rank_subset"].values()), row
    assert mg.plan_partition(128, 5, 8)[1][0] > 0 and mg.plan_partition(64, 4, 8)[1][0] > 0      # strong-scaling sizes: finest level overlaps
    assert mg.plan_partition(288, 6, 1)[1] == [0] * 6                                              # one GPU: nothing to plan
    g = pa.rank_grid(4, 2)
    h = pa.build_local_hierarchy((32, 32), 4, g, 0, 1, None, 3, [0, 3, 5, 0], "jacobi")
    assert pa.overlap_hints(h, 10) == [(False, False), (True, True), (False, True), (False, False)]   # 3 -> blocks 3,3,3,1 ; 5 -> 5,5
    h = pa.build_local_hierarchy((32, 32), 4, g, 0, 1, None, 3, [0, 11, 6, 0], "jacobi", finest_depth=2)
    assert pa.overlap_hints(h, 10) == [(False, True), (True, True), (True, True), (False, False)]
    h = pa.build_local_hierarchy((32, 32), 4, g, 0, 1, None, 3, [0, 3, 3, 0], "jacobi", sub_from=2, sub_ranks=2)
    assert pa.overlap_hints(h, 10)[1] == (True, False)            # P of level 1 reads the glued side of a redistribution: filled by it, no shortcut


@pytest.mark.gpu
def test_config4_at_full_size_through_the_host_transport(tmp_path):
    """BASELINE configs[3] as stated -- 3D Poisson Q1, 576^3 cells = 1.9e8 dofs on a 2 x 2 x 2 rank grid, 288^3 cells per rank, 6 levels --
    through `bench.py --gpus 8`'s multi-rank path, with the eight ranks sharing the one GPU of the test box over the host-staged transport
    as threads of one process (thread_ranks.py: the shared GPU machines allow few GPU processes; everything of the N = 8 run except RCCL's
    own transport, one process per rank and the timing; ~4 GB of device and ~8 GB of host memory per rank): the planner's layout (finest level own | ghost, levels 1 / 2 overlapping with depths 6 / 11, levels 3-5
    replicated), 3 CG iterations, the analytic solution to 1e-5, the exchange count of that plan."""
    import subprocess
    env = dict(os.environ, GMG_SHARE_GPU="1", GMG_TRANSPORT="host", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4",
               GMG_BENCH_DETAILS=str(tmp_path / "legs.json"))
    root = os.path.dirname(HERE)
    out = subprocess.run([sys.executable, os.path.join(HERE, "thread_ranks.py"), "8", os.path.join(root, "bench.py"), "--gpus", "8", "--cells", "288",
                          "--levels", "6", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--no-generic"],
                         env=env, cwd=root, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    assert len([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]) <= 4096
    d = json.load(open(tmp_path / "legs.json"))
    c = d["config"]
    assert d["n_gpus"] == 8 and c["dofs"] == 575 ** 3 == 190109375 and c["dofs_per_gpu"] > 2.3e7
    assert c["halo_depths"] == [0, 6, 11, 0, 0, 0] and c["replicated_from_level"] == 3
    assert c["transfer_exchanges_skipped"][1] == [True, True] and c["transfer_exchanges_skipped"][2] == [True, True]
    assert c["cg_iterations"] == 3 and c["max_abs_error_vs_exact"] < 1e-5
    # per CG iteration: 20 finest sweeps + r -= A dx + w = A p + the restriction's consistent!(r) on level 0; 2 x 2 + 1 on level 1 (depth 6:
    # blocks 6,4; the coarse correction), 2 x 1 + 1 on level 2 (depth 11) -- plus the initial residual
    assert c["halo_exchanges_per_solve"] == 3 * (23 + 5 + 3) + 1, c["halo_exchanges_per_solve"]
    assert c["transport"] == "host" and c["degraded"] is True


@pytest.mark.gpu
@pytest.mark.child_process
def test_one_rank_of_a_partition_alone_on_the_gpu(pkg):
    """multigpu._AloneTransport (tools/rank_alone.py): one rank of an 8-rank partition runs by itself -- zero halos, no peers -- so that
    its kernels can be profiled undisturbed.  The numbers mean nothing; the run must launch the partitioned path (boundary fix-ups,
    overlapping levels, replicated levels) and stay finite for a fixed number of iterations."""
    import importlib
    import torch
    mg = importlib.import_module(pkg.__name__ + ".multigpu")
    pa = importlib.import_module(pkg.__name__ + ".partition")
    rep, depths, _ = mg.plan_partition(16, 4, 8)
    g = mg.DistributedGMG((16, 16, 16), 4, 0, 8, device_id=0, transport="alone", lengths=tuple(float(v) for v in pa.rank_grid(8, 3)),
                          rep_from=rep, depth=depths, finest_depth=0)
    b = torch.from_numpy(g.rhs_lin()).cuda()
    x = torch.zeros(g.n_own, dtype=torch.float64, device="cuda")
    ex0 = g.comm_stats()[0]
    log = g.cg_solve(b, x, maxiter=3, atol=0.0, rtol=0.0)
    torch.cuda.synchronize()
    assert log.num_iters == 3 and bool(torch.isfinite(x).all()) and g.comm_stats()[0] - ex0 > 20
    assert g.comm_info()["transport"] == "host" and g.comm_info()["nranks"] == 8
    g.close()
