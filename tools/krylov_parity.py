#!/usr/bin/env python3
"""Bitwise record of a fixed list of small Krylov solves, to compare two builds of libgmgamd.so on one GPU.

Every path of the Krylov drivers (csrc/krylov.inc.hpp) and of their entry points is reached by at least one solve:

  single GMG handle   3-D Q1 Poisson 16^3, 3 levels (3375 rows), two Jacobi sweeps per smoothing pass (a GMG weak enough that no solve
                      below reaches rounding level), seeded non-zero initial guess, every
                      solve once from host and once from device memory on the same handle:
                        CG without a preconditioner, with the GMG, flexible; MINRES with and without the GMG; Richardson;
                        FGMRES(5): restarted, grown with m_add = 1 and 3 (9 iterations: the basis outgrows its caches 4 times
                        and twice), with a Jacobi Pl, each with fgmres_fused 0 and 1;
                        GMRES(5): Pr only, Pl only, Jacobi Pl + GMG Pr, neither, each restarted and grown, gmres_fused 0 and 1.
  block handle        2-D Stokes, 8 x 8 cells, 2-level velocity GMG with patch smoothers (the system of tests/krylov_block_reference.py),
                      two solves on one handle (the second reuses the caches of the first, from device memory):
                        gmg_block_fgmres_solve / gmg_block_gmres_solve (m = 3, grown) with the upper block-triangular preconditioner,
                        gmg_block_cg_solve / gmg_block_minres_solve with the SPD block-diagonal one,
                        FGMRES around upper([FGMRES(3, gmg; rtol = 1e-2), CG-Jacobi]): the nested solve (fused by default).

Per solve: iterations, flag, the residual history as the hex images of the 64-bit values, and the solution as its norm, eight
sampled entries (hex images) and the SHA-256 of its raw 64-bit image -- 130 solutions of 3375 doubles in hex would not fit a file
one wants to keep; equal digests are equal vectors.

    python tools/krylov_parity.py --out profiles/krylov_parity_branch.json [--lib /path/to/other/libgmgamd.so]
    python tools/krylov_parity.py --compare profiles/krylov_parity_parent.json profiles/krylov_parity_branch.json
--compare exits 1 unless both files hold the same solves with every entry equal."""
import argparse
import hashlib
import importlib
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOSTOP = dict(atol=1e-30, rtol=1e-30)                      # fixed iteration counts: every solve ends at its maxiter


def bits(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def record(log, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = int(log.num_iters)
    return dict(niters=n, flag=int(log.flag), hist=[bits(v) for v in np.asarray(log.residuals)[: n + 1]],
                x_norm=bits(np.linalg.norm(x)), x_sample=[bits(v) for v in x[:: max(1, x.size // 8)][:8]],
                x_sha256=hashlib.sha256(x.astype("<f8").tobytes()).hexdigest())


def solve_both(torch, S, ns, solver, b, x0, out, name):
    """host memory, then device memory, on one handle"""
    x = x0.copy()
    S.solve_(x, ns, b)
    out[name + "/host"] = record(solver.log, x)
    bd, xd = torch.from_numpy(b).cuda(), torch.from_numpy(x0.copy()).cuda()
    S.solve_(xd, ns, bd)
    torch.cuda.synchronize()
    out[name + "/device"] = record(solver.log, xd.cpu().numpy())


def single_handle(torch, pkg, out):
    S, po = pkg.solvers, pkg.poisson
    nc, nlev = (16, 16, 16), 3
    H = po.build_hierarchy(nc, nlev, 1)
    A = H["mats"][0]
    b = np.array(po.dirichlet_lift_rhs(nc, 1), dtype=np.float64)
    x0 = np.random.default_rng(5).uniform(-1.0, 1.0, b.size)

    def gmg(options=None):
        sm = [S.RichardsonSmoother(S.JacobiLinearSolver(), 2, 2.0 / 3.0)] * (nlev - 1)
        return S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sm, post_smoothers=sm, maxiter=1,
                                 mode="preconditioner", options=options)

    def run(name, solver):
        ns = S.numerical_setup(S.symbolic_setup(solver, A), A)
        solve_both(torch, S, ns, solver, b, x0, out, name)
        ns.close()

    jac = S.JacobiLinearSolver()
    run("cg/none", S.CGSolver((None, gmg()), maxiter=10, **NOSTOP))
    run("cg/gmg", S.CGSolver(gmg(), maxiter=8, **NOSTOP))
    run("cg/gmg-flexible", S.CGSolver(gmg(), maxiter=8, flexible=True, **NOSTOP))
    run("minres/none", S.MINRESSolver(Pl=(None, gmg()), maxiter=10, **NOSTOP))
    run("minres/gmg", S.MINRESSolver(Pl=gmg(), maxiter=100, atol=1e-14, rtol=1e-8))   # (past convergence dot(z, v) loses its sign)
    run("richardson/gmg", S.RichardsonLinearSolver(1.0, 6, Pl=gmg(), **NOSTOP))
    for fused in (0, 1):
        o = {"fgmres_fused": fused}
        tag = "fgmres5/fused%d/" % fused
        run(tag + "restart", S.FGMRESSolver(5, gmg(o), restart=True, maxiter=9, **NOSTOP))
        run(tag + "m_add1", S.FGMRESSolver(5, gmg(o), restart=False, m_add=1, maxiter=9, **NOSTOP))
        run(tag + "m_add3", S.FGMRESSolver(5, gmg(o), restart=False, m_add=3, maxiter=9, **NOSTOP))
        run(tag + "jacobi-pl", S.FGMRESSolver(5, gmg(o), Pl=jac, restart=True, maxiter=8, **NOSTOP))
    for fused in (0, 1):
        for grow in (False, True):
            kw = dict(restart=not grow, m_add=2, maxiter=9, **NOSTOP)
            tag = "gmres5/fused%d/%s/" % (fused, "grown" if grow else "restart")
            g = gmg({"gmres_fused": fused}); run(tag + "pr", S.GMRESSolver(5, Pr=g, **kw))
            g = gmg({"gmres_fused": fused}); run(tag + "pl", S.GMRESSolver(5, Pl=g, **kw))
            g = gmg({"gmres_fused": fused}); run(tag + "jacobi-pl+pr", S.GMRESSolver(5, Pr=g, Pl=(jac, g), **kw))
            g = gmg({"gmres_fused": fused}); run(tag + "neither", S.GMRESSolver(5, Pr=(None, g), **kw))


def block_handle(torch, pkg, out):
    S, po = pkg.solvers, pkg.poisson
    st = importlib.import_module(pkg.__name__ + ".stokes")
    alpha = 1.0e3
    sysd = st.stokes_system(8, alpha)
    Hv = st.velocity_hierarchy(8, 2, alpha)
    A = sysd["A"]
    b = np.array(sysd["b"], dtype=np.float64)
    x0 = np.random.default_rng(7).uniform(-1.0, 1.0, b.size)
    sm = [S.RichardsonSmoother(S.PatchSolver(pp, pd), 10, 0.2) for pp, pd in Hv["star_patches"]]

    def velocity_gmg(maxiter=1):
        interp = [S.PatchProlongationOperator(Hv["prolongations"][l], *Hv["interior_patches"][l], pivoting=True, rhs=Hv["graddiv"][l])
                  for l in range(len(Hv["mats"]) - 1)]
        return S.GMGLinearSolver(Hv["mats"], interp, Hv["restrictions"], pre_smoothers=sm, post_smoothers=sm,
                                 coarsest_solver=S.LUSolver(), maxiter=maxiter, mode="preconditioner")

    def upper(first):
        blocks = [[S.LinearSystemBlock(), S.LinearSystemBlock()], [S.LinearSystemBlock(), S.MatrixBlock(sysd["Mp_scaled"])]]
        cg = S.CGSolver(S.JacobiLinearSolver(), maxiter=20, atol=1e-14, rtol=1e-6)
        return S.BlockTriangularSolver(blocks, [first, cg], coeffs=[[1.0, 1.0], [0.0, 1.0]], half="upper")

    def spd_diagonal():
        # the velocity GMG made symmetric (R = P^T, one cycle) and LU(+M_p / alpha): the preconditioner of tests/test_gpu_minres.py
        def T(P):
            M = P.to_scipy().T.tocsr(); M.sort_indices()
            return po.CSR(M.shape, M.indptr, M.indices, M.data)
        g = S.GMGLinearSolver(Hv["mats"], Hv["prolongations"], [T(P) for P in Hv["prolongations"]], pre_smoothers=sm, post_smoothers=sm,
                              coarsest_solver=S.LUSolver(), maxiter=1, mode="preconditioner")
        Mp = sysd["Mp_scaled"]
        Mp = po.CSR(Mp.shape, Mp.ptr, Mp.idx, -Mp.val)
        return S.BlockDiagonalSolver([S.LinearSystemBlock(), S.MatrixBlock(Mp)], [g, S.LUSolver()])

    def run(name, solver):
        ns = S.numerical_setup(S.symbolic_setup(solver, A), A)
        x = x0.copy()
        S.solve_(x, ns, b)
        out[name + "/first-host"] = record(solver.log, x)
        bd, xd = torch.from_numpy(b).cuda(), torch.from_numpy(x0.copy()).cuda()
        S.solve_(xd, ns, bd)
        torch.cuda.synchronize()
        out[name + "/second-device"] = record(solver.log, xd.cpu().numpy())
        ns.close()

    run("block/fgmres3-upper", S.FGMRESSolver(3, upper(velocity_gmg()), restart=False, m_add=2, maxiter=6, **NOSTOP))
    run("block/gmres3-upper-pr", S.GMRESSolver(3, Pr=upper(velocity_gmg()), restart=False, m_add=2, maxiter=6, **NOSTOP))
    run("block/cg-diagonal", S.CGSolver(spd_diagonal(), maxiter=6, **NOSTOP))
    run("block/minres-diagonal", S.MINRESSolver(Pl=spd_diagonal(), maxiter=200, atol=1e-12, rtol=1e-10))
    nested = S.FGMRESSolver(3, velocity_gmg(), restart=False, m_add=1, maxiter=7, atol=1e-30, rtol=1e-2)
    run("block/fgmres3-upper-nested-fgmres3", S.FGMRESSolver(3, upper(nested), restart=True, maxiter=5, **NOSTOP))


def compare(fa, fb):
    a, b = json.load(open(fa))["solves"], json.load(open(fb))["solves"]
    bad = sorted(set(a) ^ set(b)) + [k for k in sorted(set(a) & set(b)) if a[k] != b[k]]
    for k in bad:
        print("DIFFERENT", k, a.get(k, {}).get("hist"), b.get(k, {}).get("hist"))
    print("%d solves in %s, %d in %s, %d differ" % (len(a), fa, len(b), fb, len(bad)))
    return 1 if bad or not a else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libgmgamd.so (default: this tree's)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    import torch
    import __graft_entry__ as entry
    pkg = entry.import_package()
    if a.lib:
        pkg.abi.load(os.path.abspath(a.lib))
    out = {}
    single_handle(torch, pkg, out)
    block_handle(torch, pkg, out)
    rec = dict(device=torch.cuda.get_device_name(0), solves=out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    for k, r in out.items():
        print("%-48s iters %3d flag %d  res %.3e -> %.3e" % (k, r["niters"], r["flag"], *(struct.unpack(">d", bytes.fromhex(h))[0]
                                                                                      for h in (r["hist"][0], r["hist"][-1]))))
    value = lambda h: struct.unpack(">d", bytes.fromhex(h))[0]
    bad = [k for k, r in out.items() if not all(np.isfinite(value(h)) for h in r["hist"] + [r["x_norm"]] + r["x_sample"])]
    print(json.dumps(dict(solves=len(out), nonfinite=bad)))
    sys.exit(2 if bad else 0)                               # NaN equals NaN: such a record would compare nothing


if __name__ == "__main__":
    main()
