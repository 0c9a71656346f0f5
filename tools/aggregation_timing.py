"""Smoothed-aggregation hierarchies, measured: python tools/aggregation_timing.py [--out profiles/aggregation_timing.md]
                                                                             [--cases q1,varcoef] [--levels 4] [--reps 3]

Q1 128^3 and variable-coefficient Q1 128^3 with algebraic levels only ([A0, Galerkin(), ...], [Aggregation(), ...]), from one run:
 (a) per level: rows, stored entries, rounds of the independent set, omega, the four setup times of the aggregation (HIP events,
     gmg_get_aggregation_info) next to the Galerkin times of the level below (gmg_get_galerkin_timing), and the operator complexity;
 (b) CG + GMG(Jacobi 10 / 10) to rtol 1e-8: iterations and ms per solve, against the geometric hierarchy of poisson.build_hierarchy on
     the same problem in the same process;
 (c) update() with new values (aggregates kept) against a fresh numerical setup.
--levels is chosen so that the coarsest level takes the dense inverse (the tool reports how it was built).
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

CASES = {"q1": ("Q1 128^3", (128, 128, 128), None), "varcoef": ("variable-coefficient Q1 128^3 (smooth_kappa)", (128, 128, 128), po.smooth_kappa),
         "tiny": ("Q1 16^3 (a rehearsal size: overheads only)", (16, 16, 16), None)}


def med(v):
    return float(np.median(v))


def spread(v):
    return f"{med(v):.1f} [{min(v):.1f} .. {max(v):.1f}]"


def jacobi(nlev):
    return [S.RichardsonSmoother(S.JacobiLinearSolver(), 10, 2.0 / 3.0)] * (nlev - 1)


def cg_setup(mats, interp, restrict, A0):
    import torch
    g = S.GMGLinearSolver(mats, interp, restrict, pre_smoothers=jacobi(len(mats)), post_smoothers=jacobi(len(mats)), maxiter=1)
    cg = S.CGSolver(g, maxiter=100, atol=1e-14, rtol=1e-8)
    t0 = time.perf_counter()
    ns = S.numerical_setup(S.symbolic_setup(cg, A0), A0)
    torch.cuda.synchronize()
    return cg, ns, 1e3 * (time.perf_counter() - t0)


def solves(cg, ns, b, reps):
    import torch
    bd = torch.from_numpy(b).to("cuda:0")
    t = []
    for rep in range(reps + 1):                              # round 0 is the warm-up
        xd = torch.zeros(b.size, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S.solve_(xd, ns, bd)
        torch.cuda.synchronize()
        if rep > 0:
            t.append(1e3 * (time.perf_counter() - t0))
    return cg.log.num_iters, t, xd.cpu().numpy()


def run_case(key, nlev, reps, out):
    import torch
    title, nc, kappa = CASES[key]
    A0 = po.poisson_matrix(nc, 1) if kappa is None else po.poisson_matrix_varcoef(nc, kappa)
    b = po.random_rhs(A0.shape[0])
    out.append(f"\n## {title}: {A0.shape[0]} rows, {A0.nnz} stored entries\n")
    mats = [A0] + [S.Galerkin() for _ in range(nlev - 1)]
    interp = [S.Aggregation() for _ in range(nlev - 1)]
    t_setup = []
    for rep in range(reps + 1):
        cg, ns, t = cg_setup(mats, interp, None, A0)
        if rep > 0:
            t_setup.append(t)
        if rep < reps:
            ns.close()
    g = ns.P_ns
    out.append(f"(a) {nlev} algebraic levels, Aggregation(theta=0.25); numerical setup (operators handed over + gmg_setup), ms, median "
               f"[min .. max] of {reps}: {spread(t_setup)}; coarsest solver built by `{g.coarse_info()['built_by']}`\n")
    out.append("| level | rows | stored entries | rounds | omega | strength | independent set | assignment | P | Galerkin symbolic (host) | A P | R T |")
    out.append("|---|---|---|---|---|---|---|---|---|---|---|---|")
    nnz = [A0.nnz]
    for l in range(nlev):
        rows = g.level_size(l)
        if l > 0:
            nnz.append(int(g.level_matrix(l)[3].size))
        if l == nlev - 1:
            out.append(f"| {l} | {rows} | {nnz[l]} | | | | | | | | | |")
            break
        a, q = g.aggregation_info(l), g.galerkin_timing(l + 1)
        out.append(f"| {l} | {rows} | {nnz[l]} | {a['rounds']} | {a['omega']:.4f} | {a['strength_ms']:.3f} | {a['mis_ms']:.3f} | {a['assign_ms']:.3f} | "
                   f"{a['p_ms']:.3f} | {q['symbolic_ms']:.1f} | {q['ap_ms']:.3f} | {q['rt_ms']:.3f} |")
    out.append(f"\nTimes in ms, of the last setup.  Operator complexity sum nnz(A_l) / nnz(A_0) = {sum(nnz) / nnz[0]:.3f}\n")
    it_a, t_a, x_a = solves(cg, ns, b, reps)
    # the geometric hierarchy on the same problem, in the same process
    nlev_g = 1
    while min(nc) // (2 ** nlev_g) >= 4:
        nlev_g += 1
    H = po.build_hierarchy(nc, nlev_g, 1, kappa=kappa)
    cgg, nsg, t_g_setup = cg_setup(H["mats"], H["prolongations"], H["restrictions"], H["mats"][0])
    it_g, t_g, x_g = solves(cgg, nsg, b, reps)
    nnz_g = [M.nnz for M in H["mats"]]
    nsg.close()
    out.append("(b) CG + GMG(Jacobi 10 / 10, omega 2/3) to rtol 1e-8, vectors on the device, ms per solve, median [min .. max] of %d:\n" % reps)
    out.append("| hierarchy | levels | operator complexity | setup, ms (one run) | CG iterations | ms per solve |")
    out.append("|---|---|---|---|---|---|")
    out.append(f"| aggregated | {nlev} | {sum(nnz) / nnz[0]:.3f} | {t_setup[-1]:.1f} | {it_a} | {spread(t_a)} |")
    out.append(f"| geometric (build_hierarchy) | {nlev_g} | {sum(nnz_g) / nnz_g[0]:.3f} | {t_g_setup:.1f} | {it_g} | {spread(t_g)} |")
    out.append(f"\nRelative difference of the two solutions: {np.linalg.norm(x_a - x_g) / np.linalg.norm(x_g):.1e}\n")
    # (c) value refresh against a fresh setup
    t_up = []
    for rep in range(reps + 1):
        c = 1.0 + 0.125 * (rep + 1)
        Ac = po.CSR(A0.shape, A0.ptr, A0.idx, c * A0.val)
        t0 = time.perf_counter(); S.numerical_setup_(ns, Ac); torch.cuda.synchronize()
        if rep > 0:
            t_up.append(1e3 * (time.perf_counter() - t0))
    out.append(f"(c) ms, median [min .. max] of {reps}: `update(A0')` with new values, aggregates and patterns kept: {spread(t_up)}; "
               f"a fresh numerical setup: {spread(t_setup)}")
    ns.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ge.ROOT, "profiles", "aggregation_timing.md"))
    ap.add_argument("--cases", default="q1,varcoef")
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("aggregation_timing.py needs a GPU")
    torch.zeros(1, device="cuda")
    out = ["# Smoothed-aggregation hierarchies: setup kernels, solves, value refresh",
           "",
           f"`python tools/aggregation_timing.py --cases {a.cases} --levels {a.levels} --reps {a.reps}` on {torch.cuda.get_device_name(0)}; "
           "matrices handed over whole as `poisson.CSR`.  Wall times include handing the operators over the C ABI."]
    for key in a.cases.split(","):
        run_case(key, a.levels if key != "tiny" else 3, a.reps, out)
        with open(a.out, "w") as f:                          # written after every case: a later case that fails keeps the earlier ones
            f.write("\n".join(out) + "\n")
    print("\n".join(out))


if __name__ == "__main__":
    main()
