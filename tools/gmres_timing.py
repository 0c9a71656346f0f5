#!/usr/bin/env python3
"""GMRES timing on one MI355X (b and x resident in HBM, one warm-up solve per shape, medians).

  --leg config2   Q1 128^3, 4 levels, GMG Richardson(Jacobi, 10, 2/3) pre = post: --solver gmres runs GMRES(5; Pr = GMG), --solver
                  fgmres runs FGMRES(5, GMG): iterations, ms per solve, device bytes of Krylov storage (growth of gmg_device_bytes
                  around the first solve of a handle that has already run a CG solve).
  --leg stokes    2-D Q2 / P1disc lid-driven cavity (stokes.py) at --stokes-n cells per direction with the upper block-triangular
                  preconditioner of the shipped Stokes configuration: GMRES(20; Pr = P) or FGMRES(20, P), same quantities.
  --leg columns   the Arnoldi column alone: unpreconditioned GMRES(20) without restart on the 128^3 matrix (n = 2 048 383) or, with
                  --stokes-n, on the Stokes block system; solves of k - 1 and k iterations, gmres_fused = 1 and 0 alternating in one
                  process, --reps each; column k = median T(k) - median T(k - 1) for k = 5 and 20 (Gram-Schmidt, normalisation and
                  the host round trip of the column, plus the difference in the solution update).

  --leg profile   the same solves (5 and 20 iterations, gmres_fused 1 and 0), to be run under `rocprofv3 --kernel-trace -d DIR --`;
                  --summarise DIR then reads the kernel times of that run from its database: the average stream time of every kernel
                  of the column and of the update, the stream time of a column at j = 5 and 20 (fused: one dot_partial_kernel, j
                  gmres_mgs_kernel, gmres_normalize_kernel; unfused: j + 1 dot_partial_kernel + reduce_final_kernel, j
                  axmy_dev_kernel, div_dev_kernel), gmres_combine_kernel against j axpy_kernel launches, and the achieved
                  bytes/s of gmres_mgs_kernel (4 streams x 8 n bytes) against gmg_stream_probe.

--lib PATH loads another build of libgmgamd.so (the FGMRES baseline built from the parent commit); a library without the GMRES entry
points serves --solver fgmres only.

    python tools/gmres_timing.py --leg config2 --solver gmres [--reps 20] [--out profiles/gmres_config2_gmres.json]
Prints one JSON object; --out merges it into that file under --key (default: leg, solver and size), so one file holds a whole
campaign and every entry is one run of this tool."""
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


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out)), [float(v) for v in out]


def _jac(S, nlev):
    return [S.RichardsonSmoother(S.JacobiLinearSolver(), 10, 2.0 / 3.0)] * (nlev - 1)


def _poisson(pkg):
    S, po = pkg.solvers, pkg.poisson
    nc, nlev = (128, 128, 128), 4
    H = po.build_hierarchy(nc, nlev, 1)
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=_jac(S, nlev), post_smoothers=_jac(S, nlev),
                            maxiter=1, mode="preconditioner")
    return H["mats"][0], po.dirichlet_lift_rhs(nc, 1), gmg


def _stokes(pkg, n, nlev):
    S = pkg.solvers
    st = importlib.import_module(pkg.__name__ + ".stokes")
    alpha = 1.0e3
    fast = n >= 8 and not (n & (n - 1))
    sysd = st.stokes_system_fast(n, alpha) if fast else st.stokes_system(n, alpha)
    Hv = st.velocity_hierarchy_fast(n, nlev, alpha) if fast else st.velocity_hierarchy(n, nlev, alpha)
    sm = [S.RichardsonSmoother(S.PatchSolver(pp, pd), 10, 0.2) for pp, pd in Hv["star_patches"]]
    interp = [S.PatchProlongationOperator(Hv["prolongations"][l], *Hv["interior_patches"][l], pivoting=True, rhs=Hv["graddiv"][l])
              for l in range(nlev - 1)]
    gmg = S.GMGLinearSolver(Hv["mats"], interp, Hv["restrictions"], pre_smoothers=sm, post_smoothers=sm,
                            coarsest_solver=S.LUSolver(), maxiter=4, mode="preconditioner")
    solver_p = S.CGSolver(S.JacobiLinearSolver(), maxiter=20, atol=1e-14, rtol=1e-6)
    blocks = [[S.LinearSystemBlock(), S.LinearSystemBlock()], [S.LinearSystemBlock(), S.MatrixBlock(sysd["Mp_scaled"])]]
    Pt = S.BlockTriangularSolver(blocks, [gmg, solver_p], coeffs=[[1.0, 1.0], [0.0, 1.0]], half="upper")
    return sysd["A"], sysd["b"], Pt


def solve_leg(torch, pkg, a):
    S = pkg.solvers
    if a.leg == "config2":
        A, b, P = _poisson(pkg)
        m, kw = 5, dict(maxiter=100, atol=1e-14, rtol=1e-6)
    else:
        A, b, P = _stokes(pkg, a.stokes_n, a.stokes_levels)
        m, kw = 20, dict(maxiter=100, atol=1e-10, rtol=1e-12)
    solver = S.GMRESSolver(m, Pr=P, **kw) if a.solver == "gmres" else S.FGMRESSolver(m, P, **kw)
    ns = S.numerical_setup(S.symbolic_setup(solver, A), A)
    bd = torch.from_numpy(b).cuda()
    xd = torch.zeros_like(bd)
    bytes0 = None
    if a.leg == "config2":                                  # what every solver shares is allocated by a CG solve first
        g, abi = ns.P_ns, pkg.abi
        res = abi.Result()
        abi.check(g.h, g._lib.gmg_cg_solve(g.h, C.c_void_p(bd.data_ptr()), C.c_void_p(xd.data_ptr()), abi.MEM_DEVICE, 1, 1e-14, 1e-6, 0, 1,
                                           C.byref(res), None, 0))
        torch.cuda.synchronize()
        bytes0 = g.device_bytes()

    def step():
        xd.zero_()
        S.solve_(xd, ns, bd)
    ms, runs = timed(torch, step, a.reps)
    nvec = (m + 3) if a.solver == "gmres" else (2 * m + 1)
    out = dict(leg=a.leg, solver=a.solver, m=m, dofs=int(b.size), iters=int(solver.log.num_iters), flag=int(solver.log.flag),
               ms_per_solve=ms, runs_ms=runs, krylov_vectors=nvec, krylov_vector_bytes=int(nvec * b.size * 8))
    if bytes0 is not None:
        out["krylov_device_bytes_measured"] = int(ns.P_ns.device_bytes() - bytes0)
    ns.P_ns.close()
    return out


def summarise(a):
    import glob
    import sqlite3
    f = glob.glob(os.path.join(a.summarise, "**", "*.db"), recursive=True)
    con = sqlite3.connect(f[0])
    rows = con.execute("select name, start, end from kernels order by start").fetchall()
    per = {}
    for name, s0, e0 in rows:
        for key in ("gmres_mgs_kernel", "gmres_normalize_kernel", "gmres_combine_kernel", "dot_partial_kernel", "reduce_final_kernel",
                    "axmy_dev_kernel", "div_dev_kernel", "axpy_kernel"):
            if key in name:
                per.setdefault(key, []).append((e0 - s0) / 1e3)
    n, reps = a.n, a.reps
    avg = {k: float(np.mean(v)) for k, v in per.items()}
    out = dict(leg="profile", dofs=n, launches={k: len(v) for k, v in per.items()}, avg_us=avg)
    # launch order of the profile leg: (1 + reps) fused solves of 5 iterations, then of 20: one gmres_combine_kernel each
    comb = per["gmres_combine_kernel"]
    assert len(comb) == 2 * (1 + reps), (len(comb), reps)
    c5, c20 = float(np.mean(comb[: 1 + reps])), float(np.mean(comb[1 + reps:]))
    for j, c in ((5, c5), (20, c20)):
        out["column_%d_us" % j] = dict(
            fused=avg["dot_partial_kernel"] + j * avg["gmres_mgs_kernel"] + avg["gmres_normalize_kernel"],
            unfused=(j + 1) * (avg["dot_partial_kernel"] + avg["reduce_final_kernel"]) + j * avg["axmy_dev_kernel"] + avg["div_dev_kernel"])
        out["update_%d_us" % j] = dict(gmres_combine_kernel=c, axpy_kernel_x_j=j * avg["axpy_kernel"])
    out["gmres_mgs_kernel_GBps"] = 4 * 8 * n / avg["gmres_mgs_kernel"] / 1e3
    return out


def columns_leg(torch, pkg, a):
    S, abi = pkg.solvers, pkg.abi
    if a.stokes_n:
        A, b, P = _stokes(pkg, a.stokes_n, a.stokes_levels)
    else:
        A, b, P = _poisson(pkg)
    ns = S.numerical_setup(S.symbolic_setup(S.GMRESSolver(20, Pr=(None, P)), A), A)
    g = ns.P_ns
    block = not hasattr(g, "set_option")
    fn = g._lib.gmg_block_gmres_solve if block else g._lib.gmg_gmres_solve
    chk = abi.check_block if block else abi.check
    bd = torch.from_numpy(b).cuda()
    xd = torch.zeros_like(bd)
    res = abi.Result()

    def solve(k, fused):
        if block:
            os.environ["GMG_GMRES_FUSED"] = str(fused)      # a block handle has no option table of its own: the variable is read per solve
        else:
            g.set_option("gmres_fused", fused)
        xd.zero_()
        chk(g.h, fn(g.h, C.c_void_p(bd.data_ptr()), C.c_void_p(xd.data_ptr()), abi.MEM_DEVICE, 20, 0, 1, k, 0.0, 0.0, 0, 0,
                    C.byref(res), None, 0))
        torch.cuda.synchronize()

    if a.leg == "profile":                                  # launch order summarise() relies on
        for k in (5, 20):
            for fused in (1, 0):
                for _ in range(1 + a.reps):
                    solve(k, fused)
        os.environ.pop("GMG_GMRES_FUSED", None)
        out = dict(leg="profile", dofs=int(b.size), reps=a.reps)
        probe = C.c_double()
        gh = g.block_ns[0] if block else g                  # a copy that moves the 4 x 8 n bytes of one gmres_mgs_kernel launch
        if g._lib.gmg_stream_probe(gh.h, 16 * int(b.size), 20, C.byref(probe)) == abi.OK:
            out["stream_probe_GBps"] = probe.value
        ns.P_ns.close()
        return out
    ks = (4, 5, 19, 20)
    for k in ks:
        for fused in (1, 0):
            solve(k, fused)                                 # warm-up: basis vectors, table
    t = {(k, f): [] for k in ks for f in (1, 0)}
    for _ in range(a.reps):
        for k in ks:
            for fused in (0, 1):                            # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                solve(k, fused)
                t[(k, fused)].append(1e6 * (time.perf_counter() - t0))
    os.environ.pop("GMG_GMRES_FUSED", None)
    med = {key: float(np.median(v)) for key, v in t.items()}
    out = dict(leg="columns", dofs=int(b.size), reps=a.reps, solve_us={"k%d_fused%d" % key: v for key, v in med.items()})
    for k in (5, 20):
        out["column_%d_us" % k] = dict(fused=med[(k, 1)] - med[(k - 1, 1)], unfused=med[(k, 0)] - med[(k - 1, 0)])
    probe = C.c_double()
    gh = g.block_ns[0] if block else g
    if g._lib.gmg_stream_probe(gh.h, 16 * int(b.size), 20, C.byref(probe)) == abi.OK:
        out["stream_probe_GBps"] = probe.value
    ns.P_ns.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["config2", "stokes", "columns", "profile"], default=None)
    ap.add_argument("--summarise", default=None, help="directory of a rocprofv3 --kernel-trace run of --leg profile")
    ap.add_argument("--n", type=int, default=0, help="--summarise: dofs of the profiled system")
    ap.add_argument("--key", default=None)
    ap.add_argument("--solver", choices=["gmres", "fgmres"], default="gmres")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stokes-n", type=int, default=0)
    ap.add_argument("--stokes-levels", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.leg == "stokes" and not a.stokes_n:
        a.stokes_n = 1024
    if a.summarise:
        rec = summarise(a)
        return finish(a, rec, a.key or "profile_%d" % a.n)
    import torch
    import __graft_entry__ as entry
    pkg = entry.import_package()
    if a.lib:
        probe = C.CDLL(os.path.abspath(a.lib))
        for name in ("gmg_gmres_solve", "gmg_block_gmres_solve"):
            if not hasattr(probe, name):
                pkg.abi.SYMBOLS.pop(name, None)
        pkg.abi.load(os.path.abspath(a.lib))
    t0 = time.time()
    rec = solve_leg(torch, pkg, a) if a.leg in ("config2", "stokes") else columns_leg(torch, pkg, a)
    rec["lib"] = a.lib or "this tree"
    rec["wall_s"] = time.time() - t0
    finish(a, rec, a.key or "%s_%s_%d" % (a.leg, a.solver if a.leg in ("config2", "stokes") else "gmres", rec["dofs"]))


def finish(a, rec, key):
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        allrec = json.load(open(a.out)) if os.path.exists(a.out) else {}
        allrec[key] = rec
        with open(a.out, "w") as f:
            f.write(json.dumps(allrec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
