#!/usr/bin/env python3
"""Null-space timing on one MI355X (vectors resident in HBM, warm-up per shape, medians of HIP-event times).

  --leg project   stream time of project!(.., N, x) with the subtraction x .-= p (gmg_nullspace_project, subtract = 1, no p, no alpha
                  returned: what every Krylov entry runs once when project_guess is on), nullspace_fused = 1 and 0 alternating in one
                  process, n = --cells^3 (128 and 288) and k = 1 and 6 orthonormal vectors.  The handle carries a diagonal matrix of
                  that size (only its vector length matters here).  Events are recorded on the stream the handle is pointed at
                  (gmg_set_stream), so the time is the stream's: kernels plus, on the unfused path, the idle gaps of the host round
                  trip every dot makes.  Byte model: fused (k <= 8) reads x twice and every w_k twice and writes x once,
                  (2 k + 3) 8 n bytes; unfused reads x and w_k per dot, p and w_k in and p out per axpy, p and x in and x out at the
                  end plus the memset of p: (5 k + 4) 8 n bytes.
  --leg neumann   one pure-Neumann Q1 128^3 CG + GMG solve (6 levels, coarsest 5^3 nodes solved by the constrained dense inverse,
                  NullspaceSolver(LUSolver(), N_coarse); outer NullspaceSolver(CG, N, constrain_matrix=False), rtol 1e-6) next to the
                  Dirichlet headline configuration of bench.py (128^3, 4 levels, CG rtol 1e-6) in the same process.

    python tools/nullspace_timing.py --leg project [--reps 20] [--out profiles/nullspace_timing.json]
Prints one JSON object; --out writes it to that file."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _jac(S, nlev):
    return [S.RichardsonSmoother(S.JacobiLinearSolver(), 10, 2.0 / 3.0)] * (nlev - 1)


def _diag_handle(pkg, n):
    """a 2-level GMG handle whose finest matrix is 2 I of size n (the cheapest way to a handle with vectors of length n)"""
    S, po = pkg.solvers, pkg.poisson
    nc = (n + 1) // 2
    A = po.CSR((n, n), np.arange(n + 1), np.arange(n), np.full(n, 2.0))
    P = po.CSR((n, nc), np.arange(n + 1), np.arange(n) // 2, np.ones(n))
    Ac = po.CSR((nc, nc), np.arange(nc + 1), np.arange(nc), np.full(nc, 4.0))
    gmg = S.GMGLinearSolver([A, Ac], [P], None, pre_smoothers=_jac(S, 2), post_smoothers=_jac(S, 2), maxiter=1,
                            coarsest_solver=S.CGSolver(S.JacobiLinearSolver()))
    return S.numerical_setup(S.symbolic_setup(gmg, A), A)


def leg_project(pkg, torch, cells, ks, reps):
    S, abi = pkg.solvers, pkg.abi
    out = {}
    stream = torch.cuda.Stream()
    for c in cells:
        n = c ** 3
        g = _diag_handle(pkg, n)
        g.set_stream(stream)
        rng = np.random.default_rng(1)
        x0 = torch.from_numpy(rng.standard_normal(n)).cuda()
        x = x0.clone()
        for k in ks:
            # k orthonormal vectors: indicator vectors of k interleaved index classes, normalised on the device
            V = np.zeros((k, n))
            for q in range(k):
                V[q, q::k] = 1.0
            N = S.NullSpace([V[q] for q in range(k)]).bind(g)
            S.make_orthonormal_(N)
            del V
            times = {1: [], 0: []}
            for rep in range(reps + 2):
                for fused in (1, 0):
                    g.set_option("nullspace_fused", fused)
                    x.copy_(x0)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    abi.check(g.h, g._lib.gmg_nullspace_project(g.h, C.c_void_p(x.data_ptr()), None, None, abi.MEM_DEVICE, 1))
                    e1.record(stream)
                    torch.cuda.synchronize()
                    if rep >= 2:                                     # two warm-up rounds per shape
                        times[fused].append(1e3 * e0.elapsed_time(e1))
            assert float(torch.max(torch.abs(torch.from_numpy(N.dots(x.cpu().numpy()))))) < 1e-9
            tf, tu = float(np.median(times[1])), float(np.median(times[0]))
            out[f"{c}^3 k={k}"] = dict(n=n, k=k, fused_us=tf, unfused_us=tu, ratio_unfused_over_fused=tu / tf,
                                       fused_min_us=float(np.min(times[1])), unfused_min_us=float(np.min(times[0])),
                                       model_bytes_fused=(2 * k + 3) * 8 * n, model_bytes_unfused=(5 * k + 4) * 8 * n,
                                       model_ratio=(5 * k + 4) / (2 * k + 3), fused_gbytes_per_s=(2 * k + 3) * 8 * n / tf / 1e3)
            N.unbind()
        out[f"{c}^3 stream_probe_gbytes_per_s"] = g.stream_probe(1 << 30, 10)
        g.close()
        del x, x0
    return out


def _timed_solve(S, torch, solver, A, b, reps, x0=None):
    ns = S.numerical_setup(S.symbolic_setup(solver, A), A)
    bd = torch.from_numpy(b).cuda()
    xs = torch.zeros(b.size, dtype=torch.float64, device="cuda") if x0 is None else torch.from_numpy(x0).cuda()
    xd = xs.clone()
    ts = []
    for rep in range(reps + 1):
        xd.copy_(xs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S.solve_(xd, ns, bd)
        torch.cuda.synchronize()
        if rep:
            ts.append(1e3 * (time.perf_counter() - t0))
    x = xd.cpu().numpy()
    ns.close()
    return float(np.median(ts)), x


def leg_neumann(pkg, torch, reps):
    S, po = pkg.solvers, pkg.poisson
    out = {}
    nc = (128, 128, 128)
    H = po.build_hierarchy(nc, 4, 1)
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=_jac(S, 4), post_smoothers=_jac(S, 4),
                            coarsest_solver=S.LUSolver(), maxiter=1, mode="preconditioner")
    cg = S.CGSolver(gmg, maxiter=20, atol=1e-14, rtol=1e-6)
    b = po.dirichlet_lift_rhs(nc, 1)
    ms, x = _timed_solve(S, torch, cg, H["mats"][0], b, reps)
    out["dirichlet 128^3, 4 levels"] = dict(dofs=int(b.size), iterations=cg.log.num_iters, flag=cg.log.flag, ms=ms)
    del H
    nlev = 6
    H = po.neumann_hierarchy(nc, nlev, 1)
    nL = H["mats"][-1].shape[0]
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=_jac(S, nlev), post_smoothers=_jac(S, nlev),
                            coarsest_solver=S.NullspaceSolver(S.LUSolver(), S.NullSpace(np.ones(nL))), maxiter=1, mode="preconditioner")
    cg = S.CGSolver(gmg, maxiter=20, atol=1e-14, rtol=1e-6)
    A = H["mats"][0]
    n = A.shape[0]
    b = po.neumann_rhs(nc)
    x0 = np.random.default_rng(1).standard_normal(n)
    ms, x = _timed_solve(S, torch, S.NullspaceSolver(cg, S.NullSpace(np.ones(n)), constrain_matrix=False), A, b, reps, x0)
    res = float(np.linalg.norm(A.matvec(x) - b) / np.linalg.norm(b))
    out[f"neumann 128^3, {nlev} levels"] = dict(dofs=n, coarsest_dofs=nL, iterations=cg.log.num_iters, flag=cg.log.flag, ms=ms,
                                                rel_residual=res, x_dot_ones=float(x.sum()), x0_dot_ones=float(x0.sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["project", "neumann"], required=True)
    ap.add_argument("--cells", default="128,288")
    ap.add_argument("--k", default="1,6")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path to time"
    import __graft_entry__ as entry
    pkg = entry.import_package()
    if args.leg == "project":
        res = leg_project(pkg, torch, [int(c) for c in args.cells.split(",")], [int(k) for k in args.k.split(",")], args.reps)
    else:
        res = leg_neumann(pkg, torch, max(3, args.reps // 4))
    res = {args.leg: res}
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
