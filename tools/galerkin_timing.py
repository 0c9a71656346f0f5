"""Galerkin coarse matrices, measured: python tools/galerkin_timing.py [--out profiles/galerkin_timing.md] [--cases q1,q2] [--reps 3]

Q1 128^3 with 4 levels and Q2 64^3 with 4 levels, from one run:
 (a) the numerical setup (operators handed over + gmg_setup, wall time ending in a device synchronise) with the coarse matrices given
     against Galerkin levels, alternating, the first round discarded as warm-up;
 (b) the two product launches per level (HIP events, gmg_get_galerkin_timing) and the host symbolic phase against scipy's
     R @ (A @ P) on the host;
 (c) update() with the finest matrix alone (Galerkin levels follow) against update() with the matrices of all levels passed.
Needs a GPU: there is no CPU path."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as ge

pkg = ge.import_package()
S, po = pkg.solvers, pkg.poisson

CASES = {"q1": ("Q1 128^3, 4 levels", (128, 128, 128), 4, 1), "q2": ("Q2 64^3, 4 levels", (64, 64, 64), 4, 2),
         "tiny": ("Q1 16^3, 3 levels (a rehearsal size: overheads only)", (16, 16, 16), 3, 1)}


def med(v):
    return float(np.median(v))


def spread(v):
    return f"{med(v):.1f} [{min(v):.1f} .. {max(v):.1f}]"


def run_case(key, reps, out):
    import torch
    title, nc, nlev, order = CASES[key]
    H = po.build_hierarchy(nc, nlev, order)
    mats, Ps, Rs = H["mats"], H["prolongations"], H["restrictions"]
    sm = [S.RichardsonSmoother(S.JacobiLinearSolver(), 10, 2.0 / 3.0)] * (nlev - 1)
    gal = [mats[0]] + [S.Galerkin() for _ in range(nlev - 1)]

    def setup(smatrices):
        g = S.GMGLinearSolver(smatrices, Ps, Rs, pre_smoothers=sm, post_smoothers=sm, maxiter=1)
        t0 = time.perf_counter()
        ns = S.numerical_setup(S.symbolic_setup(g, smatrices[0]), smatrices[0])
        torch.cuda.synchronize()
        return ns, 1e3 * (time.perf_counter() - t0)

    t_given, t_gal, kern = [], [], []
    for rep in range(reps + 1):                              # alternating; round 0 is the warm-up
        ns, t = setup(mats)
        ns.close()
        ng, tg = setup(gal)
        if rep > 0:
            t_given.append(t)
            t_gal.append(tg)
            kern.append([ng.galerkin_timing(l) for l in range(1, nlev)])
        if rep < reps:
            ng.close()
    out.append(f"\n## {title} ({mats[0].shape[0]} rows, {mats[0].nnz} stored entries on level 0)\n")
    out.append("(a) numerical setup, ms, median [min .. max] of %d:\n" % reps)
    out.append(f"- coarse matrices given: {spread(t_given)}")
    out.append(f"- Galerkin levels: {spread(t_gal)}\n")
    out.append("(b) per Galerkin level, ms (median of the same runs); scipy = `R @ (A @ P)` on the host, one run:\n")
    out.append("| level | rows | stored entries | symbolic (host) | T = A P (device) | R T (device) | scipy (host) | max abs diff / max abs |")
    out.append("|---|---|---|---|---|---|---|---|")
    A = mats[0].to_scipy().tocsr()
    for l in range(1, nlev):
        shape, ptr, idx, val = ng.level_matrix(l)
        P, R = Ps[l - 1].to_scipy().tocsr(), Rs[l - 1].to_scipy().tocsr()
        t0 = time.perf_counter()
        C = (R @ (A @ P)).tocsr()
        t_sp = 1e3 * (time.perf_counter() - t0)
        G = po.CSR(shape, ptr, idx, val).to_scipy()
        err = abs(G - C).max() / abs(C).max()
        k = [r[l - 1] for r in kern]
        out.append(f"| {l} | {shape[0]} | {val.size} | {med([q['symbolic_ms'] for q in k]):.1f} | {med([q['ap_ms'] for q in k]):.3f} | "
                   f"{med([q['rt_ms'] for q in k]):.3f} | {t_sp:.1f} | {err:.1e} |")
        A = G.tocsr()                                        # the chain: the next level is formed from this one
    # (c) value refresh: the same patterns, every value scaled (the structure of the hierarchy is kept)
    nm, _t = setup(mats)
    t_one, t_all = [], []
    for rep in range(reps + 1):
        c = 1.0 + 0.125 * (rep + 1)
        scaled = [po.CSR(M.shape, M.ptr, M.idx, c * M.val) for M in mats]
        t0 = time.perf_counter(); ng.update(scaled[0]); torch.cuda.synchronize()
        a = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter(); nm.update(scaled[0], scaled); torch.cuda.synchronize()
        b = 1e3 * (time.perf_counter() - t0)
        if rep > 0:
            t_one.append(a)
            t_all.append(b)
    out.append(f"\n(c) `update()`, ms, median [min .. max] of {reps}:\n")
    out.append(f"- one matrix, Galerkin levels follow (symbolic phase kept): {spread(t_one)}")
    out.append(f"- the matrices of all levels passed: {spread(t_all)}")
    b = np.random.default_rng(5).standard_normal(mats[0].shape[0])
    xg, xm = np.zeros_like(b), np.zeros_like(b)
    S.solve_(xg, ng, b)
    S.solve_(xm, nm, b)
    out.append(f"\nOne V-cycle after the last update, Galerkin against given matrices: relative difference {np.linalg.norm(xg - xm) / np.linalg.norm(xm):.1e}")
    ng.close()
    nm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ge.ROOT, "profiles", "galerkin_timing.md"))
    ap.add_argument("--cases", default="q1,q2")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("galerkin_timing.py needs a GPU")
    torch.zeros(1, device="cuda")
    out = ["# Galerkin coarse matrices: setup, product kernels, value refresh",
           "",
           f"`python tools/galerkin_timing.py --cases {a.cases} --reps {a.reps}` on {torch.cuda.get_device_name(0)}; Jacobi 10 / 10 smoothers, "
           "matrices handed over whole as `poisson.CSR`.  Wall times include handing the operators over the C ABI."]
    for key in a.cases.split(","):
        run_case(key, a.reps, out)
        with open(a.out, "w") as f:                          # written after every case: a later case that fails keeps the earlier ones
            f.write("\n".join(out) + "\n")
    print("\n".join(out))


if __name__ == "__main__":
    main()
