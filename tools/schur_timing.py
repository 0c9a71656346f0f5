#!/usr/bin/env python3
"""Schur complement preconditioner against the upper block-triangular one on one MI355X: 2-D Q2 / P1disc lid-driven cavity
(stokes.py) at --stokes-n cells per direction (default 1024), the velocity GMG of the shipped Stokes configuration (vertex-star patch
smoothers Richardson(PatchSolver, 10, 0.2), patch prolongation with the grad-div rhs, LU coarsest, maxiter = 4) and
CGSolver(JacobiLinearSolver(); maxiter = 20, rtol = 1e-6) on -1/alpha M_p in both, FGMRES(20; atol = 1e-10, rtol = 1e-12).  b and x
are resident in HBM.

  --leg solve     both preconditioners set up in one process; after one warm-up solve each, --reps solves alternating between the
                  two, each between device synchronisations: outer iterations, median ms per solve, and the median ms of one
                  application of each preconditioner alone (gmg_block_precond_apply on device vectors).
  --leg profile   to be run under `rocprofv3 --kernel-trace -d DIR --`: 1 + --reps applications of the Schur preconditioner alone,
                  each preceded by a one-element torch kernel that marks its start in the trace.
  --summarise DIR reads that trace: the kernels of one application are A-solve, y_p - C x_u, S-solve, B x_p, A-solve, x_u - du
                  (SchurComplementSolvers.jl:65-71).  The two A-solves launch the same kernels, so the three seam passes are found
                  by position: the last kernel, and the two that follow / precede the longest common prefix / suffix run.  Reports
                  their stream time and its share of the stream time of all kernels of the application (medians over --reps).

    python tools/schur_timing.py --leg solve [--reps 10] [--out profiles/schur_timing.json]
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


def _gmg(S, Hv, nlev):
    sm = [S.RichardsonSmoother(S.PatchSolver(pp, pd), 10, 0.2) for pp, pd in Hv["star_patches"]]
    interp = [S.PatchProlongationOperator(Hv["prolongations"][l], *Hv["interior_patches"][l], pivoting=True, rhs=Hv["graddiv"][l])
              for l in range(nlev - 1)]
    return S.GMGLinearSolver(Hv["mats"], interp, Hv["restrictions"], pre_smoothers=sm, post_smoothers=sm,
                             coarsest_solver=S.LUSolver(), maxiter=4, mode="preconditioner")


def _cg_p(S):
    return S.CGSolver(S.JacobiLinearSolver(), maxiter=20, atol=1e-14, rtol=1e-6)


def triangular(S, sysd, Hv, nlev):
    blocks = [[S.LinearSystemBlock(), S.LinearSystemBlock()], [S.LinearSystemBlock(), S.MatrixBlock(sysd["Mp_scaled"])]]
    return S.BlockTriangularSolver(blocks, [_gmg(S, Hv, nlev), _cg_p(S)], coeffs=[[1.0, 1.0], [0.0, 1.0]], half="upper")


def schur(S, sysd, Hv, nlev):
    return S.SchurComplementSolver((_gmg(S, Hv, nlev), None), sysd["A"][0][1], sysd["A"][1][0], (_cg_p(S), sysd["Mp_scaled"]))


def _apply(abi, g, bd, xd):
    abi.check_block(g.h, g._lib.gmg_block_precond_apply(g.h, C.c_void_p(bd.data_ptr()), C.c_void_p(xd.data_ptr()), abi.MEM_DEVICE))


def solve_leg(torch, pkg, a):
    S, abi = pkg.solvers, pkg.abi
    sysd, Hv = _inputs(pkg, a.stokes_n, a.stokes_levels)
    b = sysd["b"]
    bd = torch.from_numpy(b).cuda()
    xd = torch.zeros_like(bd)
    runs = {}
    for name, make in (("triangular", triangular), ("schur", schur)):
        solver = S.FGMRESSolver(20, make(S, sysd, Hv, a.stokes_levels), **KW)
        runs[name] = dict(solver=solver, ns=S.numerical_setup(S.symbolic_setup(solver, sysd["A"]), sysd["A"]), solve=[], apply=[])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def solve(r):
        xd.zero_()
        S.solve_(xd, r["ns"], bd)

    def apply(r):
        xd.zero_()
        _apply(abi, r["ns"].P_ns, bd, xd)

    for r in runs.values():                                 # warm-up: code objects, Krylov basis, block caches
        solve(r); apply(r)
    torch.cuda.synchronize()
    for _ in range(a.reps):                                 # alternating: what else runs on the host hits both alike
        for r in runs.values():
            r["solve"].append(timed(lambda: solve(r)))
    for _ in range(a.reps):
        for r in runs.values():
            r["apply"].append(timed(lambda: apply(r)))
    out = dict(leg="solve", n=a.stokes_n, levels=a.stokes_levels, dofs=int(b.size), sizes=[int(v) for v in sysd["sizes"]], reps=a.reps, m=20)
    for name, r in runs.items():
        solve(r)                                            # the logs of a whole solve (the applications above overwrote the block logs)
        torch.cuda.synchronize()
        log = r["solver"].log
        res = float(np.linalg.norm(sysd["K"] @ xd.cpu().numpy() - b)) if "K" in sysd and sysd["K"] is not None else None
        out[name] = dict(iters=int(log.num_iters), flag=int(log.flag), final_residual_estimate=float(log.residuals[log.num_iters]),
                         true_residual=res, ms_per_solve=float(np.median(r["solve"])), solve_runs_ms=[float(v) for v in r["solve"]],
                         ms_per_iteration=float(np.median(r["solve"])) / max(1, int(log.num_iters)),
                         ms_per_application=float(np.median(r["apply"])), apply_runs_ms=[float(v) for v in r["apply"]],
                         block_solver_iters=[int(sv.log.num_iters) for sv in r["solver"].Pr.solvers])
        r["ns"].P_ns.close()
    return out


def profile_leg(torch, pkg, a):
    S, abi = pkg.solvers, pkg.abi
    sysd, Hv = _inputs(pkg, a.stokes_n, a.stokes_levels)
    P = schur(S, sysd, Hv, a.stokes_levels)
    ns = S.numerical_setup(S.symbolic_setup(P, sysd["A"]), sysd["A"])
    bd = torch.from_numpy(sysd["b"]).cuda()
    xd = torch.zeros_like(bd)
    mark = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(1 + a.reps):
        xd.zero_()
        torch.cuda.synchronize()
        mark.add_(1)                                        # the marker: a torch elementwise kernel, no kernel of the library
        torch.cuda.synchronize()
        _apply(abi, ns, bd, xd)
        torch.cuda.synchronize()
    mark.add_(1)
    torch.cuda.synchronize()
    ns._fill_logs()
    out = dict(leg="profile", n=a.stokes_n, dofs=int(sysd["b"].size), reps=a.reps, block_solver_iters=[int(sv.log.num_iters) for sv in P.solvers])
    ns.close()
    return out


def summarise(a):
    import glob
    import sqlite3
    f = sorted(glob.glob(os.path.join(a.summarise, "**", "*.db"), recursive=True))
    con = sqlite3.connect(f[0])
    rows = con.execute("select name, start, end from kernels order by start").fetchall()
    marks = [i for i, (name, _s, _e) in enumerate(rows) if "elementwise" in name and "gmg" not in name]
    # torch's kernels (the marker and the fill of x before it) cut the trace; an application is a run of library kernels between two cuts
    apps = []
    for i0, i1 in zip(marks[:-1], marks[1:]):
        seg = [r for r in rows[i0 + 1:i1] if "at::native" not in r[0] and "elementwise" not in r[0]]
        if len(seg) > 8:
            apps.append(seg)
    apps = apps[1:]                                         # the first application is the warm-up
    assert apps, "no application found between the markers"
    per = []
    for seg in apps:
        names = [r[0] for r in seg]
        L = len(names)
        m = next(k for k in range((L - 3) // 2, 0, -1) if names[:k] == names[L - 1 - k:L - 1])
        seams = dict(resid_C=seg[m], set_B=seg[L - 2 - m], axpy=seg[L - 1])
        busy = sum(e - s for _n, s, e in seg) / 1e3
        per.append(dict(kernels=L, a_solve_kernels=m, s_solve_kernels=L - 3 - 2 * m, busy_us=busy, span_us=(seg[-1][2] - seg[0][1]) / 1e3,
                        seam_us={k: (v[2] - v[1]) / 1e3 for k, v in seams.items()}, seam_kernels={k: v[0][:120] for k, v in seams.items()},
                        a_solve_us=[sum(e - s for _n, s, e in seg[:m]) / 1e3, sum(e - s for _n, s, e in seg[L - 1 - m:L - 1]) / 1e3],
                        s_solve_us=sum(e - s for _n, s, e in seg[m + 1:L - 2 - m]) / 1e3))
    med = lambda v: float(np.median(v))
    seam = {k: med([p["seam_us"][k] for p in per]) for k in ("resid_C", "set_B", "axpy")}
    busy = med([p["busy_us"] for p in per])
    return dict(leg="profile_summary", applications=len(per), kernels_per_application=per[0]["kernels"],
                a_solve_kernels=per[0]["a_solve_kernels"], s_solve_kernels=per[0]["s_solve_kernels"], seam_kernels=per[0]["seam_kernels"],
                seam_us=seam, seam_total_us=sum(seam.values()), stream_busy_us=busy, span_us=med([p["span_us"] for p in per]),
                seam_share_of_stream_time=sum(seam.values()) / busy,
                a_solve_us=[med([p["a_solve_us"][i] for p in per]) for i in (0, 1)], s_solve_us=med([p["s_solve_us"] for p in per]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["solve", "profile"], default=None)
    ap.add_argument("--summarise", default=None, help="directory of a rocprofv3 --kernel-trace run of --leg profile")
    ap.add_argument("--key", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--stokes-n", type=int, default=1024)
    ap.add_argument("--stokes-levels", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.summarise:
        return finish(a, summarise(a), a.key or "profile_summary_%d" % a.stokes_n)
    if not a.leg:
        ap.error("--leg or --summarise")
    import torch
    import __graft_entry__ as entry
    if not torch.cuda.is_available():
        sys.exit("schur_timing.py measures on the GPU: no device visible")
    pkg = entry.import_package()
    t0 = time.time()
    rec = solve_leg(torch, pkg, a) if a.leg == "solve" else profile_leg(torch, pkg, a)
    rec["wall_s"] = time.time() - t0
    finish(a, rec, a.key or "%s_%d" % (a.leg, a.stokes_n))


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
