#!/usr/bin/env python3
"""What the Chebyshev smoother costs on a partitioned hierarchy against the Richardson smoother over the same M, on one MI355X, one
process, the variants ALTERNATING call by call (medians of --reps, at least five, with minimum and maximum).

  q1      3-D Poisson Q1 at --cells per direction (default 64), --levels levels (default 4), the partition of --ranks ranks (default 8,
          2 x 2 x 2) folded onto the one GPU (partition.fold_ranks), every halo exchange and all-reduce through RCCL (transport
          rccl_loopback): CG + GMG with ChebyshevSmoother(Jacobi, 3, eig_method = "lanczos") against RichardsonSmoother(Jacobi, 10, 2/3),
          pre = post, rtol 1e-8
  q2      Q2 at --q2-cells per direction (default 8), --q2-levels levels (default 2), folded W = 8, vertex-star patches owned per rank:
          FGMRES(5) + GMG with ChebyshevSmoother(patch, 4) against RichardsonSmoother(patch, 10, 0.2), rtol 1e-6
  per case: ms per solve, ms per V-cycle (the GMG as a preconditioner), iterations, halo exchanges per V-cycle, lambda_est per level
  pack_ab option cheb_pack_fused 1 against 0 on level 0 of the Chebyshev handle, alternating: one pass (gmg_smooth on device vectors)
          between two device synchronisations, per sweep = pass / degree; the bits of both settings compared

The loopback's self messages (56 per exchange on 2 x 2 x 2) dominate such runs: these are FUNCTIONAL figures of the partitioned code
path on one GPU, not scaling figures.

    python tools/chebyshev_dist_timing.py [--cells 64] [--levels 4] [--ranks 8] [--reps 7] [--out X.json] [--md profiles/chebyshev_dist_timing.md]
Prints one JSON object; --md also writes the tables as markdown."""
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


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--q2-cells", type=int, default=8)
    ap.add_argument("--q2-levels", type=int, default=2)
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--transport", default="rccl_loopback")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    assert a.reps >= 5, "medians of at least five runs"
    import torch
    import __graft_entry__ as entry
    pkg = entry.import_package()
    po, abi = pkg.poisson, pkg.abi
    pa, mg = (importlib.import_module(pkg.__name__ + "." + m) for m in ("partition", "multigpu"))
    if not torch.cuda.is_available():
        sys.exit("chebyshev_dist_timing.py measures on the GPU: no device visible")
    W = a.ranks

    def sync_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def alternating(fns):
        for f in fns.values():
            f()                                               # warm-up: code objects, work vectors
        t = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, f in fns.items():
                t[k].append(sync_ms(f))
        return {k: _stats(v) for k, v in t.items()}

    def case(nc, nlev, order, variants, solve, rtol):
        grid = pa.rank_grid(W, 3)
        F = pa.fold_ranks([pa.build_local_hierarchy(nc, nlev, grid, r, order, None, None, None, "jacobi") for r in range(W)])
        tabs = pa.fold_patch_tables(F) if order == 2 else None
        gid = F["levels"][0].own_gid
        b = torch.from_numpy(np.ascontiguousarray(po.dirichlet_lift_rhs(nc, order)[gid])).cuda()
        hs, logs = {}, {}
        for name, kw in variants.items():
            hs[name] = mg.DistributedGMG(nc, nlev, 0, 2, device_id=0, transport=a.transport, local_hierarchy=F, cells_global=nc, order=order,
                                         patch_tables=tabs, **kw)
        x = torch.zeros_like(b)

        def solver(name):
            def run():
                x.zero_()
                g = hs[name]
                logs[name] = g.cg_solve(b, x, maxiter=50, atol=1e-14, rtol=rtol) if solve == "cg" else \
                    g.fgmres_solve(b, x, m=5, maxiter=50, atol=1e-14, rtol=rtol)
            return run

        res = dict(cells=nc[0], levels=nlev, order=order, ranks=W, dofs=int(F["levels"][0].n_own), solver=solve, rtol=rtol)
        res["solve_ms"] = alternating({k: solver(k) for k in hs})
        res["iterations"] = {k: int(logs[k].num_iters) for k in hs}
        res["vcycle_ms"] = alternating({k: (lambda g=g: g.apply(b, x)) for k, g in hs.items()})
        res["exchanges_per_vcycle"] = {}
        for k, g in hs.items():
            e0 = g.comm_stats()[0]
            g.apply(b, x)
            torch.cuda.synchronize()
            res["exchanges_per_vcycle"][k] = g.comm_stats()[0] - e0
        gc = hs["chebyshev"]
        res["lambda_est"] = [gc.chebyshev_info(l)["lambda_est"] for l in range(nlev - 1)]
        res["pack_fused_level0"] = bool(gc.halo_info(0)["pack_fused"])
        degree = gc.chebyshev_info(0)["degree"]
        # ---- cheb_pack_fused 1 against 0: one pass of level 0
        n0 = F["levels"][0].n_own
        r0 = torch.from_numpy(np.random.default_rng(0).uniform(-1.0, 1.0, n0)).cuda()
        bits, t = {}, {1: [], 0: []}
        for rep in range(a.reps + 1):                         # (the first round is the warm-up)
            for fused in (1, 0):
                abi.check(gc.h, gc._lib.gmg_set_option(gc.h, b"cheb_pack_fused", float(fused)))
                xx, rr = torch.zeros_like(r0), r0.clone()
                ms = sync_ms(lambda: abi.check(gc.h, gc._lib.gmg_smooth(gc.h, 0, abi.PRE, C.c_void_p(xx.data_ptr()), C.c_void_p(rr.data_ptr()), abi.MEM_DEVICE)))
                bits[fused] = (xx, rr)
                if rep:
                    t[fused].append(ms)
        abi.check(gc.h, gc._lib.gmg_set_option(gc.h, b"cheb_pack_fused", 1.0))
        res["pack_ab"] = dict(pass_ms={"cheb_pack_fused_%d" % k: _stats(v) for k, v in t.items()},
                              per_sweep_ms={"cheb_pack_fused_%d" % k: float(np.median(v)) / degree for k, v in t.items()},
                              same_bits=bool(torch.equal(bits[0][0], bits[1][0]) and torch.equal(bits[0][1], bits[1][1])))
        for g in hs.values():
            g.close()
        return res

    out = dict(transport=a.transport, reps=a.reps)
    out["q1"] = case((a.cells,) * 3, a.levels, 1,
                     dict(chebyshev=dict(smoother="jacobi", chebyshev=dict(degree=3, eig_method="lanczos")),
                          richardson=dict(smoother="jacobi", niter=10, omega=2.0 / 3.0)), "cg", 1e-8)
    out["q2"] = case((a.q2_cells,) * 3, a.q2_levels, 2,
                     dict(chebyshev=dict(smoother="patch", chebyshev=dict(degree=4)),
                          richardson=dict(smoother="patch", niter=10, omega=0.2)), "fgmres", 1e-6)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(out))
    print(json.dumps(out))


def markdown(out):
    fmt = lambda s: "%.3f (%.3f .. %.3f)" % (s["median"], s["min"], s["max"])
    lines = ["# Chebyshev smoother on partitioned levels: timings", "",
             "`tools/chebyshev_dist_timing.py`, one MI355X, one process, transport `%s`, the variants alternating call by call, medians of %d "
             "(minimum .. maximum).  A W-rank partition folded onto one GPU sends every message to itself (56 self messages per exchange on "
             "2 x 2 x 2), and that dominates these runs: the figures are **functional figures** of the partitioned code path, **not scaling "
             "figures**." % (out["transport"], out["reps"]), ""]
    for key, title in (("q1", "Q1, CG + GMG, Chebyshev(Jacobi, 3, lanczos) against Richardson(Jacobi, 10, 2/3)"),
                       ("q2", "Q2, FGMRES(5) + GMG, Chebyshev(patch, 4) against Richardson(patch, 10, 0.2)")):
        c = out[key]
        lines += ["## %s" % title, "",
                  "%d^3 cells, %d levels, W = %d folded, %d owned dofs on level 0, rtol %g.  lambda_est per level: %s.  Pack fused on level 0: %s." %
                  (c["cells"], c["levels"], c["ranks"], c["dofs"], c["rtol"], ", ".join("%.4f" % v for v in c["lambda_est"]), c["pack_fused_level0"]), "",
                  "| variant | iterations | ms per solve | ms per V-cycle | halo exchanges per V-cycle |", "|---|---|---|---|---|"]
        for v in ("chebyshev", "richardson"):
            lines.append("| %s | %d | %s | %s | %d |" % (v, c["iterations"][v], fmt(c["solve_ms"][v]), fmt(c["vcycle_ms"][v]), c["exchanges_per_vcycle"][v]))
        p = c["pack_ab"]
        lines += ["", "| `cheb_pack_fused` | ms per pass of level 0 | ms per sweep | same bits |", "|---|---|---|---|"]
        for k in (1, 0):
            lines.append("| %d | %s | %.4f | %s |" % (k, fmt(p["pass_ms"]["cheb_pack_fused_%d" % k]), p["per_sweep_ms"]["cheb_pack_fused_%d" % k], p["same_bits"]))
        lines.append("")
    return "\n".join(lines)


if __name__ == "__main__":
    main()
