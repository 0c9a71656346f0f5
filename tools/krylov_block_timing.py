#!/usr/bin/env python3
"""A Krylov solver around the velocity GMG as a block solver (FGMRESSolver(20, gmg) as solvers[1] of the upper block-triangular
preconditioner, test/Applications/NavierStokesGMG.jl:159-169) against the bare GMG, on one MI355X.  b and x are resident in HBM.

  --leg stokes   2-D Q2 / P1disc lid-driven cavity (stokes.py) at --stokes-n cells per direction (default 1024: config 5), the velocity
                 GMG of the shipped configuration (vertex-star patch smoothers, patch prolongation with the grad-div rhs, LU coarsest,
                 maxiter = 4), CG-Jacobi on -1/alpha M_p; the symmetric system and the one whose velocity block carries a seeded
                 relative perturbation of --rel on every entry (same pattern, nonsymmetric).  Under FGMRES(20; atol = 1e-10, rtol =
                 1e-12, maxiter = --outer-maxiter):
                     base          upper([gmg, CG-Jacobi])                                     -- the path before this solver existed
                     nested        upper([FGMRES(20, gmg; rtol, maxiter = 20), CG-Jacobi])     rtol = 1e-8 and 1e-2, fgmres_fused 0 and 1
                 All handles live in one process; after one warm-up solve each, --reps solves alternate between them.  Records outer
                 iterations, nested applications and iterations (gmg_block_diag_stats), median seconds per solve.
  --leg share    what of a nested solve is not V-cycles: one application of BlockDiagonalSolver([FGMRES(20, gmg; maxiter = k, no stop)])
                 on the velocity block alone, fgmres_fused 0 and 1, against k applications of BlockDiagonalSolver([gmg]) -- the rest is
                 the k + 1 mat-vecs, the Arnoldi columns and the solution update; the difference between fused and unfused is the
                 Arnoldi column and update alone.  --problem stokes | q1 (the Q1 Poisson hierarchy at --q1-cells, default 128, Jacobi
                 smoothers: where the V-cycle is cheapest and Arnoldi should weigh most).

    python tools/krylov_block_timing.py --leg stokes [--reps 5] [--out profiles/krylov_block_timing.json]
Prints one JSON object; --out merges it into that file under --key (default: the leg and the size)."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KW = dict(maxiter=100, atol=1e-10, rtol=1e-12)


def _inputs(pkg, n, nlev):
    st = importlib.import_module(pkg.__name__ + ".stokes")
    alpha = 1.0e3
    fast = n >= 8 and not (n & (n - 1))
    sysd = st.stokes_system_fast(n, alpha) if fast else st.stokes_system(n, alpha)
    Hv = st.velocity_hierarchy_fast(n, nlev, alpha) if fast else st.velocity_hierarchy(n, nlev, alpha)
    return sysd, Hv


def _perturbed(po, M, seed, rel):
    u = np.random.default_rng([seed, M.val.size]).uniform(-1.0, 1.0, M.val.size)
    return po.CSR(M.shape, M.ptr, M.idx, M.val * (1.0 + rel * u))


def _gmg(S, Hv, mats, nlev, options=None):
    sm = [S.RichardsonSmoother(S.PatchSolver(pp, pd), 10, 0.2) for pp, pd in Hv["star_patches"]]
    interp = [S.PatchProlongationOperator(Hv["prolongations"][l], *Hv["interior_patches"][l], pivoting=True, rhs=Hv["graddiv"][l])
              for l in range(nlev - 1)]
    return S.GMGLinearSolver(mats, interp, Hv["restrictions"], pre_smoothers=sm, post_smoothers=sm,
                             coarsest_solver=S.LUSolver(), maxiter=4, mode="preconditioner", options=options)


def _q1_gmg(S, H, options=None):
    nlev = len(H["mats"])
    sm = [S.RichardsonSmoother(S.JacobiLinearSolver(), 10, 2.0 / 3.0)] * (nlev - 1)
    return S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sm, post_smoothers=sm, maxiter=1,
                             mode="preconditioner", options=options)


def _say(*a):
    print(*a, file=sys.stderr, flush=True)


def _timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _stats(run):
    v = np.array(run)
    return dict(median_s=float(np.median(v)), min_s=float(v.min()), max_s=float(v.max()), runs_s=[float(x) for x in v])


def stokes_leg(torch, pkg, a):
    S, po = pkg.solvers, pkg.poisson
    sysd, Hv = _inputs(pkg, a.stokes_n, a.stokes_levels)
    _say("inputs assembled")
    nlev = a.stokes_levels
    out = dict(leg="stokes", n=a.stokes_n, levels=nlev, dofs=int(sysd["b"].size), sizes=[int(v) for v in sysd["sizes"]], reps=a.reps,
               rel=a.rel, outer=dict(KW, m=20, maxiter=a.outer_maxiter), inner=dict(m=20, maxiter=20, atol=1e-12))
    bd = torch.from_numpy(np.array(sysd["b"])).cuda()
    xd = torch.zeros_like(bd)
    for variant in a.variants.split(","):
        A = [list(r) for r in sysd["A"]]
        if variant == "perturbed":
            A[0][0] = _perturbed(po, A[0][0], 55, a.rel)
        mats = [A[0][0]] + list(Hv["mats"][1:])
        blocks = [[S.LinearSystemBlock(), S.LinearSystemBlock()], [S.LinearSystemBlock(), S.MatrixBlock(sysd["Mp_scaled"])]]
        cgp = lambda: S.CGSolver(S.JacobiLinearSolver(), maxiter=20, atol=1e-14, rtol=1e-6)
        runs = {}

        def add(name, sv):
            P = S.BlockTriangularSolver(blocks, [sv, cgp()], coeffs=[[1.0, 1.0], [0.0, 1.0]], half="upper")
            solver = S.FGMRESSolver(20, P, **dict(KW, maxiter=a.outer_maxiter))
            t0 = time.perf_counter()
            ns = S.numerical_setup(S.symbolic_setup(solver, A), A)
            runs[name] = dict(solver=solver, ns=ns, t=[], setup_s=time.perf_counter() - t0)
            _say("[%s] %s set up in %.1f s" % (variant, name, runs[name]["setup_s"]))

        add("base", _gmg(S, Hv, mats, nlev))
        for rtol in (1e-8, 1e-2):
            for fused in (0, 1):
                add("nested_rtol%g_fused%d" % (rtol, fused),
                    S.FGMRESSolver(20, _gmg(S, Hv, mats, nlev, {"fgmres_fused": fused}), maxiter=20, atol=1e-12, rtol=rtol))

        def solve(r):
            xd.zero_()
            S.solve_(xd, r["ns"], bd)

        for r in runs.values():                              # warm-up: code objects, Krylov bases, block caches
            r["warm_s"] = _timed(torch, lambda: solve(r))
            _say("[%s] warm-up solve %.3f s, %d outer iterations" % (variant, r["warm_s"], r["solver"].log.num_iters))
        reps = a.reps if max(r["warm_s"] for r in runs.values()) < a.max_solve_s else 1   # (a solve that does not converge is timed once)
        for _ in range(reps):                                # alternating: what else runs on the host hits all alike
            for r in runs.values():
                r["t"].append(_timed(torch, lambda: solve(r)))
            _say("[%s] repetition done" % variant)
        rec = {}
        for name, r in runs.items():
            app0, it0 = r["ns"].P_ns.diag_stats(0)           # (the statistics count from the setup: one more solve, the difference)
            solve(r)
            torch.cuda.synchronize()
            log = r["solver"].log
            napp, nit = (v - w for v, w in zip(r["ns"].P_ns.diag_stats(0), (app0, it0)))
            rec[name] = dict(outer_iters=int(log.num_iters), flag=int(log.flag), final_residual_estimate=float(log.residuals[log.num_iters]),
                             inner_applications=napp, inner_iters=nit, setup_s=r["setup_s"], warm_s=r["warm_s"], **_stats(r["t"]))
            r["ns"].P_ns.close()
        out[variant] = rec
        _merge(a, a.key or "stokes_%d" % a.stokes_n, out)     # (a variant that is done is on record whatever happens to the next)
    return out


def share_leg(torch, pkg, a):
    S, po, abi = pkg.solvers, pkg.poisson, pkg.abi
    k = a.k
    if a.problem == "stokes":
        sysd, Hv = _inputs(pkg, a.stokes_n, a.stokes_levels)
        A = sysd["A"][0][0]
        mats = [A] + list(Hv["mats"][1:])
        gmg = lambda opt=None: _gmg(S, Hv, mats, a.stokes_levels, opt)
        size = a.stokes_n
    else:
        H = po.build_hierarchy((a.q1_cells,) * 3, a.q1_levels, 1)
        A = H["mats"][0]
        gmg = lambda opt=None: _q1_gmg(S, H, opt)
        size = a.q1_cells
    n = int(A.shape[0])
    # a new right-hand side per application: the nested solve starts from the handle's own y (the previous solution), so the same
    # right-hand side again would iterate on rounding noise
    bs = [torch.from_numpy(np.random.default_rng(q).uniform(-1, 1, n)).cuda() for q in range(a.reps + 1)]
    xd = torch.zeros_like(bs[0])
    runs = {"gmg": S.BlockDiagonalSolver([gmg()])}
    for fused in (0, 1):
        runs["fgmres_fused%d" % fused] = S.BlockDiagonalSolver([S.FGMRESSolver(20, gmg({"fgmres_fused": fused}), maxiter=k, atol=1e-300, rtol=1e-300)])
    ns = {name: S.numerical_setup(S.symbolic_setup(P, [[A]]), [[A]]) for name, P in runs.items()}
    t = {name: [] for name in runs}

    def apply(name, bd):
        g = ns[name]
        for _ in range(k if name == "gmg" else 1):
            abi.check_block(g.h, g._lib.gmg_block_precond_apply(g.h, C.c_void_p(bd.data_ptr()), C.c_void_p(xd.data_ptr()), abi.MEM_DEVICE))

    for name in runs:
        apply(name, bs[0])
    for q in range(a.reps):
        for name in runs:
            t[name].append(_timed(torch, lambda: apply(name, bs[q + 1])))
    out = dict(leg="share", problem=a.problem, size=size, rows=n, k=k, reps=a.reps)
    for name in runs:
        out[name] = _stats(t[name])
    vc = out["gmg"]["median_s"]
    for fused in (0, 1):
        T = out["fgmres_fused%d" % fused]["median_s"]
        out["fgmres_fused%d" % fused]["non_vcycle_share"] = 1.0 - vc / T
        out["fgmres_fused%d" % fused]["inner_applications_and_iters"] = list(ns["fgmres_fused%d" % fused].diag_stats(0))
    out["fused_minus_unfused_s"] = out["fgmres_fused1"]["median_s"] - out["fgmres_fused0"]["median_s"]
    for g in ns.values():
        g.close()
    return out


def _merge(a, key, rec):
    if not a.out:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    allrec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    allrec[key] = rec
    with open(a.out, "w") as f:
        f.write(json.dumps(allrec, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["stokes", "share"], required=True)
    ap.add_argument("--key", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stokes-n", type=int, default=1024)
    ap.add_argument("--stokes-levels", type=int, default=7)
    ap.add_argument("--variants", default="symmetric,perturbed")
    ap.add_argument("--rel", type=float, default=1.0e-3)
    ap.add_argument("--outer-maxiter", type=int, default=60)
    ap.add_argument("--max-solve-s", type=float, default=5.0, help="--leg stokes: above this warm-up time every solver is timed once, not --reps times")
    ap.add_argument("--problem", choices=["stokes", "q1"], default="q1")
    ap.add_argument("--q1-cells", type=int, default=128)
    ap.add_argument("--q1-levels", type=int, default=4)
    ap.add_argument("--k", type=int, default=10, help="--leg share: iterations of the nested solve")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    if not torch.cuda.is_available():
        sys.exit("krylov_block_timing.py measures on the GPU: no device visible")
    pkg = entry.import_package()
    t0 = time.time()
    rec = stokes_leg(torch, pkg, a) if a.leg == "stokes" else share_leg(torch, pkg, a)
    rec["wall_s"] = time.time() - t0
    key = a.key or ("stokes_%d" % a.stokes_n if a.leg == "stokes" else "share_%s_%d" % (a.problem, rec["size"]))
    _merge(a, key, rec)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
