#!/usr/bin/env python3
"""MINRES vs CG / FGMRES timing on one MI355X (device events, warmed-up shapes, b and x resident in HBM).

  config 2   Q1 128^3, 4 levels, GMG Richardson(Jacobi, 10, 2/3) pre = post: CGSolver(gmg) and MINRESSolver(Pl=gmg) on ONE handle
             (gmg_cg_solve / gmg_minres_solve with use_precond = 1): iterations, ms per solve, us per iteration.
  Stokes     2-D Q2 / P1disc lid-driven cavity (stokes.py) at --stokes-n cells per direction:
             FGMRES(20) + upper block-triangular preconditioner (the shipped config 5), and
             MINRES + BlockDiagonalSolver([velocity GMG, Jacobi on +M_p / alpha]) with a symmetric velocity GMG (patch smoother
             pre = post, the plain P with R = P^T, one V-cycle): iterations, ms per solve, device bytes.

    python tools/minres_timing.py [--reps 5] [--stokes-n 1024] [--stokes-levels 7] [--skip-stokes] [--out profiles/minres_timing.json]
Prints one JSON object; --out also writes it."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, reps):
    """median device time of fn() over reps runs (one event pair each), after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), [float(v) for v in out]


def config2(torch, pkg, reps):
    import ctypes as C
    S, po, abi = pkg.solvers, pkg.poisson, pkg.abi
    nc, nlev = (128, 128, 128), 4
    H = po.build_hierarchy(nc, nlev, 1)
    sm = [S.RichardsonSmoother(S.JacobiLinearSolver(), 10, 2.0 / 3.0)] * (nlev - 1)
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sm, post_smoothers=sm,
                            maxiter=1, mode="preconditioner")
    A = H["mats"][0]
    ns = S.numerical_setup(S.symbolic_setup(S.CGSolver(gmg), A), A)
    g = ns.P_ns
    b = po.dirichlet_lift_rhs(nc, 1)
    bd = torch.from_numpy(b).cuda()
    xd = torch.zeros_like(bd)
    res = abi.Result()
    hist = np.zeros(101)
    args = (C.c_void_p(bd.data_ptr()), C.c_void_p(xd.data_ptr()), abi.MEM_DEVICE, 100, 1e-14, 1e-6)
    tail = (C.byref(res), C.c_void_p(hist.ctypes.data), hist.size)

    def cg():
        xd.zero_()
        abi.check(g.h, g._lib.gmg_cg_solve(g.h, *args, 0, 1, *tail))

    def minres():
        xd.zero_()
        abi.check(g.h, g._lib.gmg_minres_solve(g.h, *args, 1, *tail))

    out = {}
    for name, fn in (("cg", cg), ("minres", minres)):
        ms, runs = timed(torch, fn, reps)
        r = xd.cpu().numpy()
        out[name] = dict(iters=int(res.niters), flag=int(res.flag), ms_per_solve=ms, us_per_iter=1e3 * ms / max(1, res.niters),
                         runs_ms=runs, res0=float(res.res0), res=float(res.res),
                         l2err=float(po.l2_error_sq(nc, 1, r)))
    out["minres_over_cg_per_iter"] = out["minres"]["us_per_iter"] / out["cg"]["us_per_iter"]
    out["device_bytes"] = g.device_bytes()
    g.close()
    return out


def stokes(torch, pkg, n, nlev, reps):
    S, po = pkg.solvers, pkg.poisson
    st = importlib.import_module(pkg.__name__ + ".stokes")
    alpha = 1.0e3
    fast = n >= 8 and not (n & (n - 1))
    sysd = st.stokes_system_fast(n, alpha) if fast else st.stokes_system(n, alpha)
    Hv = st.velocity_hierarchy_fast(n, nlev, alpha) if fast else st.velocity_hierarchy(n, nlev, alpha)
    b = sysd["b"]
    nu, npp = sysd["sizes"]
    bd = torch.from_numpy(b).cuda()
    xd = torch.zeros_like(bd)
    Ab = sysd["A"]

    def resid():
        x = xd.cpu().numpy()
        ru = Ab[0][0].matvec(x[:nu]) + Ab[0][1].matvec(x[nu:]) - b[:nu]
        rp = Ab[1][0].matvec(x[:nu]) - b[nu:]
        return float(np.sqrt(ru @ ru + rp @ rp))

    def run(solver, gmg):
        ns = S.numerical_setup(S.symbolic_setup(solver, sysd["A"]), sysd["A"])

        def step():
            xd.zero_()
            S.solve_(xd, ns, bd)
        ms, runs = timed(torch, step, reps)
        gv = ns.P_ns.block_ns[0]
        N = b.size
        nvec = (2 * solver.m + 1) if isinstance(solver, S.FGMRESSolver) else 9
        r = dict(iters=int(solver.log.num_iters), flag=int(solver.log.flag), ms_per_solve=ms, runs_ms=runs,
                 residual=resid(), velocity_gmg_device_bytes=int(gv.device_bytes()), krylov_vectors=nvec,
                 krylov_vector_bytes=int(nvec * N * 8))
        ns.P_ns.close()
        return r

    # (a) the shipped config 5: FGMRES(20) + upper block-triangular, GMG(maxiter 4, patch prolongation), CG-Jacobi pressure block
    sm = [S.RichardsonSmoother(S.PatchSolver(pp, pd), 10, 0.2) for pp, pd in Hv["star_patches"]]
    interp = [S.PatchProlongationOperator(Hv["prolongations"][l], *Hv["interior_patches"][l], pivoting=True, rhs=Hv["graddiv"][l])
              for l in range(nlev - 1)]
    gmg = S.GMGLinearSolver(Hv["mats"], interp, Hv["restrictions"], pre_smoothers=sm, post_smoothers=sm,
                            coarsest_solver=S.LUSolver(), maxiter=4, mode="preconditioner")
    solver_p = S.CGSolver(S.JacobiLinearSolver(), maxiter=20, atol=1e-14, rtol=1e-6)
    blocks = [[S.LinearSystemBlock(), S.LinearSystemBlock()], [S.LinearSystemBlock(), S.MatrixBlock(sysd["Mp_scaled"])]]
    Pt = S.BlockTriangularSolver(blocks, [gmg, solver_p], coeffs=[[1.0, 1.0], [0.0, 1.0]], half="upper")
    out = {"n": n, "levels": nlev, "dofs": int(b.size)}
    out["fgmres20_block_triangular"] = run(S.FGMRESSolver(20, Pt, atol=1e-10, rtol=1e-12, maxiter=100), gmg)
    # (b) MINRES + BlockDiagonalSolver([symmetric velocity GMG, Jacobi on +M_p / alpha])
    Ps = Hv["prolongations"]
    Rs = []
    for P in Ps:
        T = P.to_scipy().T.tocsr()
        T.sort_indices()
        Rs.append(po.CSR(T.shape, T.indptr, T.indices, T.data))
    sm = [S.RichardsonSmoother(S.PatchSolver(pp, pd), 10, 0.2) for pp, pd in Hv["star_patches"]]
    gmg_s = S.GMGLinearSolver(Hv["mats"], Ps, Rs, pre_smoothers=sm, post_smoothers=sm, coarsest_solver=S.LUSolver(), maxiter=1,
                              mode="preconditioner")
    Mp = sysd["Mp_scaled"].to_scipy() * -1.0
    Mp = Mp.tocsr()
    Mp.sort_indices()
    Pd = S.BlockDiagonalSolver([S.LinearSystemBlock(), S.MatrixBlock(po.CSR(Mp.shape, Mp.indptr, Mp.indices, Mp.data))],
                               [gmg_s, S.JacobiLinearSolver()])
    out["minres_block_diagonal"] = run(S.MINRESSolver(Pl=Pd, atol=1e-10, rtol=1e-12, maxiter=1000), gmg_s)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stokes-n", type=int, default=1024)
    ap.add_argument("--stokes-levels", type=int, default=7)
    ap.add_argument("--skip-stokes", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    pkg = entry.import_package()
    t0 = time.time()
    rec = {}

    def save():
        rec["wall_s"] = time.time() - t0
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(rec, indent=1) + "\n")
    rec["config2"] = config2(torch, pkg, a.reps)
    save()
    if not a.skip_stokes:
        rec["stokes"] = stokes(torch, pkg, a.stokes_n, a.stokes_levels, max(2, a.reps // 2))
        save()
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
