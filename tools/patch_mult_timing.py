#!/usr/bin/env python3
"""What the MultiplicativePatchSmoother costs and buys on one MI355X against the additive patch smoothers, everything in one process,
vectors resident in HBM (the protocol of tools/chebyshev_timing.py).

  solve     3-D Poisson Q2 at --cells per direction (default 64), --levels GMG levels (default 4), vertex-star patches on every level,
            matrices handed over whole (every leg has a CSR), Dirichlet-lift rhs, FGMRES(5) and CG to rtol 1e-6 with
              richardson_10   RichardsonSmoother(PatchSolver, 10, 0.2) pre = post
              chebyshev_4     ChebyshevSmoother(PatchSolver, 4) pre = post
              pmult_fwd_bwd   MultiplicativePatchSmoother, 1 forward sweep pre + 1 backward sweep post
              pmult_sym       MultiplicativePatchSmoother, 1 symmetric sweep pre = post
            per leg: iterations, ms per solve, ms per smoothing pass (gmg_smooth) and per patch sweep on level 0, launches per pass
            (profiled; the multiplicative legs), device bytes, seconds of numerical_setup
  one       pmult_one_launch 0 (one launch per colour) against 2 (the whole pass as one launch of one workgroup): ms per forward pass
            on the two-level Q2 problems of --small-cells (meshes such as 8x8 or 6x6x6), to place the default of pmult_one_launch_max

The legs alternate inside every round; one warm-up round, then --reps rounds (default 5), each call between two device
synchronisations; medians, minima and maxima are kept.

    python tools/patch_mult_timing.py [--cells 64] [--levels 4] [--reps 5] [--small-cells 4x4,8x8,4x4x4,...]
                                      [--out profiles/patch_mult_timing.md] [--json profiles/patch_mult_timing.json]
Prints one JSON object and writes the two files."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small-cells", default="4x4,8x8,4x4x4,12x12,6x6x6,8x8x8,12x12x12,16x16x16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_mult_timing.md"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "patch_mult_timing.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    if not torch.cuda.is_available():
        sys.exit("patch_mult_timing.py measures on the GPU: no device visible")
    pkg = entry.import_package()
    S, po = pkg.solvers, pkg.poisson

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def alternate(fns):
        ms = {k: [] for k in fns}
        for rep in range(a.reps + 1):
            for k, fn in fns.items():
                t = timed(fn)
                if rep:
                    ms[k].append(t)
        return {k: _stats(v) for k, v in ms.items()}

    def legs(Ms):
        """name -> (pre, post, patch sweeps per pass of the pre-smoother)"""
        rich = [S.RichardsonSmoother(M, 10, 0.2) for M in Ms]
        cheb = [S.ChebyshevSmoother(M, 4) for M in Ms]
        fwd = [S.MultiplicativePatchSmoother(M, 1, 1.0, "forward") for M in Ms]
        bwd = [S.MultiplicativePatchSmoother(M, 1, 1.0, "backward") for M in Ms]
        sym = [S.MultiplicativePatchSmoother(M, 1, 1.0, "symmetric") for M in Ms]
        return {"richardson_10": (rich, rich, 10), "chebyshev_4": (cheb, cheb, 4), "pmult_fwd_bwd": (fwd, bwd, 1), "pmult_sym": (sym, sym, 2)}

    out = dict(reps=a.reps)
    # ---------------------------------------------------------------- the solves
    nc, nlev, order = (a.cells,) * 3, a.levels, 2
    H = po.build_hierarchy(nc, nlev, order, stream_min_rows=1 << 40)
    Ms = [S.PatchSolver(*po.vertex_star_patches(H["ncells"][l], order)) for l in range(nlev - 1)]
    bd = torch.from_numpy(po.dirichlet_lift_rhs(nc, order)).cuda()
    xd = torch.zeros_like(bd)
    n0 = int(H["mats"][0].shape[0])
    rs = torch.from_numpy(np.random.default_rng(0).uniform(-1.0, 1.0, n0)).cuda()
    xs, rw = torch.zeros_like(rs), torch.zeros_like(rs)
    sv = dict(cells=a.cells, levels=nlev, dofs=[int(M.shape[0]) for M in H["mats"]], patches=[int(M.patch_ptr.size - 1) for M in Ms],
              setup_s={}, device_bytes={}, sweeps_per_pass={}, launches_per_pass={}, colors={}, signature_level0={})
    for krylov in ("fgmres", "cg"):
        handles, solves, passes = {}, {}, {}
        for name, (pre, post, sweeps) in legs(Ms).items():
            gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=pre, post_smoothers=post, maxiter=1)
            kw = dict(maxiter=50, atol=1e-14, rtol=1e-6)
            solver = S.FGMRESSolver(5, gmg, **kw) if krylov == "fgmres" else S.CGSolver(gmg, **kw)
            t0 = time.perf_counter()
            ns = S.numerical_setup(S.symbolic_setup(solver, H["mats"][0]), H["mats"][0])
            torch.cuda.synchronize()
            if krylov == "fgmres":
                sv["setup_s"][name] = time.perf_counter() - t0
                sv["device_bytes"][name] = int(ns.P_ns.device_bytes())
                sv["sweeps_per_pass"][name] = sweeps
                if name.startswith("pmult"):
                    sv["colors"][name] = [int(ns.P_ns.patch_coloring(l)[0]) for l in range(nlev - 1)]
            handles[name] = (ns, solver)

            def solve(ns=ns):
                xd.zero_()
                S.solve_(xd, ns, bd)

            def one_pass(ns=ns):
                xs.zero_(); rw.copy_(rs)
                ns.P_ns.smooth(0, xs, rw)

            solves[name], passes[name] = solve, one_pass
        sv[krylov + "_solve_ms"] = alternate(solves)
        sv[krylov + "_iters"] = {name: int(solver.log.num_iters) for name, (_ns, solver) in handles.items()}
        sv[krylov + "_flag"] = {name: int(solver.log.flag) for name, (_ns, solver) in handles.items()}
        if krylov == "fgmres":
            sv["pass_ms"] = alternate(passes)
            sv["copy_ms"] = alternate(dict(copy=lambda: (xs.zero_(), rw.copy_(rs))))["copy"]       # what one_pass spends outside the library
            sv["sweep_ms"] = {k: (v["median"] - sv["copy_ms"]["median"]) / sv["sweeps_per_pass"][k] for k, v in sv["pass_ms"].items()}
            for name, (ns, _s) in handles.items():
                sv["signature_level0"][name] = ns.P_ns.sweep_signature(0)
                if name.startswith("pmult"):
                    ns.P_ns.profile(0)
                    passes[name]()
                    sv["launches_per_pass"][name] = int(ns.P_ns.kernel_stats()["launches"])
                    ns.P_ns.profile(0, False)
        for ns, _s in handles.values():
            ns.P_ns.close()
    out["solve"] = sv
    # ---------------------------------------------------------------- one launch per colour against one launch per pass
    ol = []
    for mesh in [q for q in a.small_cells.split(",") if q]:
        cells = tuple(int(v) for v in mesh.split("x"))
        Hs = po.build_hierarchy(cells, 2, order)
        M = S.PatchSolver(*po.vertex_star_patches(cells, order))
        sm = [S.MultiplicativePatchSmoother(M, 1, 1.0, "forward")]
        gmg = S.GMGLinearSolver(Hs["mats"], Hs["prolongations"], Hs["restrictions"], pre_smoothers=sm, post_smoothers=sm, maxiter=1)
        ns = S.numerical_setup(S.symbolic_setup(gmg, Hs["mats"][0]), Hs["mats"][0])
        n = int(Hs["mats"][0].shape[0])
        r1 = torch.from_numpy(np.random.default_rng(1).uniform(-1.0, 1.0, n)).cuda()
        x1, w1 = torch.zeros_like(r1), torch.zeros_like(r1)

        def run(mode, ns=ns, x1=x1, w1=w1, r1=r1):
            ns.set_option("pmult_one_launch", mode)
            x1.zero_(); w1.copy_(r1)
            ns.smooth(0, x1, w1)

        t = alternate({"per_colour": lambda: run(0), "one_launch": lambda: run(2)})
        ol.append(dict(cells=mesh, dofs=n, patches=int(M.patch_ptr.size - 1), colors=int(ns.patch_coloring(0)[0]),
                       per_colour_ms=t["per_colour"], one_launch_ms=t["one_launch"]))
        ns.close()
    out["one_launch"] = ol
    # ---------------------------------------------------------------- the files
    lines = ["# MultiplicativePatchSmoother against the additive patch smoothers on one MI355X", "",
             "Written by `tools/patch_mult_timing.py`; medians of %d alternating rounds after one warm-up round (min .. max in brackets)." % a.reps, "",
             "## Q2 %d^3, %d levels, rtol 1e-6, Dirichlet-lift rhs" % (a.cells, nlev), "",
             "dofs per level: %s; patches per smoothed level: %s; colours per level: %s" % (sv["dofs"], sv["patches"], json.dumps(sv["colors"])), "",
             "| smoother | FGMRES(5) its | ms per solve | CG its | ms per solve | ms per pass (level 0) | ms per patch sweep | launches per pass | device GB | setup s |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for k in sv["fgmres_solve_ms"]:
        f, c = sv["fgmres_solve_ms"][k], sv["cg_solve_ms"][k]
        lines.append("| %s | %d | %.2f (%.2f .. %.2f) | %d | %.2f (%.2f .. %.2f) | %.3f | %.3f | %s | %.2f | %.2f |" % (
            k, sv["fgmres_iters"][k], f["median"], f["min"], f["max"], sv["cg_iters"][k], c["median"], c["min"], c["max"],
            sv["pass_ms"][k]["median"], sv["sweep_ms"][k], sv["launches_per_pass"].get(k, "-"), sv["device_bytes"][k] / 1e9, sv["setup_s"][k]))
    lines.extend(["", "A pass is one gmg_smooth call of the pre-smoother on level 0 (x = 0, a copy of r: %.3f ms, subtracted before the division by "
                  "the patch sweeps of the pass: 10, 4, 1 and 2).  Launches per pass: profiled (colour launches + the x update; r -= A dx not "
                  "counted); not recorded for the additive legs.  Level-0 signatures: %s" % (sv["copy_ms"]["median"], json.dumps(sv["signature_level0"])), "",
                  "## pmult_one_launch: one launch per colour (0) against the whole pass as one launch of one workgroup (2)", "",
                  "Two-level Q2 problems, one forward pass on level 0 (gmg_smooth, x = 0).", "",
                  "| cells | dofs | patches | colours | per colour ms | one launch ms |", "|---|---|---|---|---|---|"])
    for q in ol:
        lines.append("| %s | %d | %d | %d | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) |" % (
            q["cells"], q["dofs"], q["patches"], q["colors"], q["per_colour_ms"]["median"], q["per_colour_ms"]["min"], q["per_colour_ms"]["max"],
            q["one_launch_ms"]["median"], q["one_launch_ms"]["min"], q["one_launch_ms"]["max"]))
    lines.append("")
    for path, text in ((a.out, "\n".join(lines) + "\n"), (a.json, json.dumps(out, indent=1) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
