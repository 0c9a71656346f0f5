#!/usr/bin/env python3
"""What numerical_setup! of a block solver costs on one MI355X against a fresh numerical_setup, everything in one process.

Problems: the Stokes system of config 5 (gridapsolvers.jl_amd/stokes.py: Q2 velocity / discontinuous P1 pressure, grad-div form,
FGMRES(20) with the upper block-triangular preconditioner [GMG (vertex-star patch smoothers, 4 cycles)  B^T ; 0  CG-Jacobi on the
scaled pressure mass matrix]) at --cells cells per direction (default 256 and 1024).  The operator has constant coefficients, whose
device layouts are dictionaries chosen from the values; the three system blocks get a seeded relative perturbation (1e-6 on the
velocity block, 1e-9 on the gradient and divergence blocks, two value sets) so that every block is stored with explicit values and the
in-place path is taken -- what a Navier-Stokes Jacobian gives by itself.  The velocity block is a NonlinearSystemBlock.

  fresh_setup_s   numerical_setup(symbolic_setup(solver, A), A), --reps times, each on a new handle
  refresh_s       numerical_setup_(ns, A') alternating between the two value sets, --reps times, with its stages:
                    record      the values copied to the handle's host blocks (gmg_block_update_values)
                    gmg         the velocity GMG handle's own refresh (gmg_update_values + gmg_setup: its finest level, patch blocks)
                    block_setup gmg_block_setup, and from GMG_SETUP_TIMING=1 on stderr its host-to-device copies, refills and inverses
  solve_ms        one solve!(x, ns, b) from x = 0 before the first and after the last refresh, with iteration counts
Every figure: median, minimum and maximum.  The refill kernel's A/B is tools/mb_refill.hip (profiles/mb_refill.txt).

    python tools/block_refresh_timing.py [--cells 256,1024] [--reps 5] [--out profiles/block_refresh_timing]
Writes <out>.json and <out>.md and prints the JSON object."""
import argparse
import importlib
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


class _Stderr:
    """what the library writes to file descriptor 2 inside the block"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    if not torch.cuda.is_available():
        sys.exit("block_refresh_timing.py measures on the GPU: no device visible")
    os.environ["GMG_SETUP_TIMING"] = "1"
    pkg = entry.import_package()
    S, po = pkg.solvers, pkg.poisson
    st = importlib.import_module(pkg.__name__ + ".stokes")
    alpha = 1.0e3

    def perturbed(M, seed, rel):
        u = np.random.default_rng([seed, M.val.size]).uniform(-1.0, 1.0, M.val.size)
        return po.CSR(M.shape, M.ptr, M.idx, M.val * (1.0 + rel * u))

    out = dict(reps=a.reps, problems=[])
    for n in [int(c) for c in a.cells.split(",")]:
        nlev = {256: 5, 1024: 7}.get(n, max(2, int(np.log2(n)) - 3))
        sysd = st.stokes_system_fast(n, alpha)
        Hv = st.velocity_hierarchy_fast(n, nlev, alpha)
        A0 = sysd["A"]
        sets = [[[perturbed(A0[0][0], 10 + k, 1e-6), perturbed(A0[0][1], 20 + k, 1e-9)], [perturbed(A0[1][0], 30 + k, 1e-9), None]] for k in (0, 1)]

        def make():
            sm = [S.RichardsonSmoother(S.PatchSolver(pp, pd), 10, 0.2) for pp, pd in Hv["star_patches"]]
            interp = [S.PatchProlongationOperator(Hv["prolongations"][l], *Hv["interior_patches"][l], pivoting=True, rhs=Hv["graddiv"][l])
                      for l in range(nlev - 1)]
            gmg = S.GMGLinearSolver(Hv["mats"], interp, Hv["restrictions"], pre_smoothers=sm, post_smoothers=sm,
                                    coarsest_solver=S.LUSolver(), maxiter=4, mode="preconditioner")
            solver_p = S.CGSolver(S.JacobiLinearSolver(), maxiter=20, atol=1e-14, rtol=1e-6)
            blocks = [[S.NonlinearSystemBlock(), S.LinearSystemBlock()], [S.LinearSystemBlock(), S.MatrixBlock(sysd["Mp_scaled"])]]
            Pd = S.BlockTriangularSolver(blocks, [gmg, solver_p], coeffs=[[1.0, 1.0], [0.0, 1.0]], half="upper")
            return S.FGMRESSolver(20, Pd, atol=1e-10, rtol=1e-12, maxiter=100)

        bd = torch.from_numpy(sysd["b"]).cuda()
        xd = torch.zeros_like(bd)
        fresh = []
        ns = solver = None
        with _Stderr() as err_fresh:
            for _ in range(a.reps):
                if ns is not None:
                    ns.P_ns.close()
                solver = make()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ns = S.numerical_setup(S.symbolic_setup(solver, sets[0]), sets[0])
                torch.cuda.synchronize()
                fresh.append(time.perf_counter() - t0)

        def solves():
            ms = []
            for r in range(a.reps + 1):
                xd.zero_(); torch.cuda.synchronize()
                t0 = time.perf_counter()
                S.solve_(xd, ns, bd)
                torch.cuda.synchronize()
                if r:
                    ms.append(1e3 * (time.perf_counter() - t0))
            return dict(ms=_stats(ms), iters=int(solver.log.num_iters), flag=int(solver.log.flag))

        solve_before = solves()
        bytes0 = ns.P_ns.setup_info()["device_bytes"]
        refresh, stages, lib_lines = [], [], []
        for r in range(a.reps):
            with _Stderr() as err:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                S.numerical_setup_(ns, sets[(r + 1) % 2])
                torch.cuda.synchronize()
                refresh.append(time.perf_counter() - t0)
            stages.append(dict(ns.P_ns.update_seconds))
            lib_lines.append([l for l in err.text.splitlines() if l.startswith("[gmg")])
        info = ns.P_ns.setup_info()
        solve_after = solves()
        m = [re.search(r"copy\s+([\d.]+) ms, refill \(\+ D\^-1\)\s+([\d.]+) ms, inverses\s+([\d.]+) ms, total\s+([\d.]+) ms", "\n".join(ls)) for ls in lib_lines]
        g = [re.search(r"\[gmg_setup\] value refresh\s+([\d.]+) ms", "\n".join(ls)) for ls in lib_lines]
        prob = dict(cells=n, levels=nlev, sizes=[int(v) for v in sysd["sizes"]],
                    nnz=dict(A_uu=int(A0[0][0].val.size), A_up=int(A0[0][1].val.size), A_pu=int(A0[1][0].val.size)),
                    fresh_setup_s=_stats(fresh), refresh_s=_stats(refresh),
                    refresh_stages_s={k: _stats([s[k] for s in stages]) for k in stages[0]},
                    block_setup_ms=dict(h2d_copy=_stats([float(x.group(1)) for x in m if x]), refill=_stats([float(x.group(2)) for x in m if x]),
                                        inverses=_stats([float(x.group(3)) for x in m if x]), total=_stats([float(x.group(4)) for x in m if x]))
                    if all(m) else None,
                    gmg_value_refresh_ms=_stats([float(x.group(1)) for x in g if x]) if all(g) else None,
                    gmg_refresh_in_place=bool(all(g)), setup_info=info, device_bytes_before=bytes0,
                    solve_before=solve_before, solve_after=solve_after, library_lines_last_refresh=lib_lines[-1][-12:])
        out["problems"].append(prob)
        ns.P_ns.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + ".json", "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        with open(a.out + ".md", "w") as f:
            f.write("# numerical_setup! of the block solver against a fresh numerical_setup (tools/block_refresh_timing.py)\n\n")
            f.write("Stokes system of config 5, one MI355X, %d repetitions each (median [min .. max]).  The three system blocks carry a seeded relative\n"
                    "perturbation (1e-6 velocity, 1e-9 gradient / divergence) so that their layouts hold explicit values; the velocity block is a\n"
                    "NonlinearSystemBlock.  Refill kernel A/B: profiles/mb_refill.txt.\n\n" % a.reps)
            fm = lambda s, u=1.0, d=3: "%.*f [%.*f .. %.*f]" % (d, u * s["median"], d, u * s["min"], d, u * s["max"])
            for p in out["problems"]:
                f.write("## %d x %d cells, %d levels (%d + %d dofs; nnz %s)\n\n" % (p["cells"], p["cells"], p["levels"], p["sizes"][0], p["sizes"][1], p["nnz"]))
                f.write("| | seconds |\n|---|---|\n")
                f.write("| fresh numerical_setup | %s |\n| numerical_setup! (kind %d, %d blocks, %.1f MB of values) | %s |\n" %
                        (fm(p["fresh_setup_s"]), p["setup_info"]["kind"], p["setup_info"]["blocks_refreshed"], p["setup_info"]["value_bytes"] / 1e6, fm(p["refresh_s"])))
                for k, v in p["refresh_stages_s"].items():
                    f.write("| -- %s | %s |\n" % (k, fm(v, 1.0, 4)))
                if p["block_setup_ms"]:
                    for k, v in p["block_setup_ms"].items():
                        f.write("| ---- gmg_block_setup: %s (ms) | %s |\n" % (k, fm(v, 1.0, 2)))
                if p["gmg_value_refresh_ms"]:
                    f.write("| ---- velocity GMG handle: value refresh (ms) | %s |\n" % fm(p["gmg_value_refresh_ms"], 1.0, 1))
                else:
                    f.write("| ---- velocity GMG handle | full set-up (a level in a value-dependent layout) |\n")
                f.write("| solve before (ms, %d iterations) | %s |\n| solve after (ms, %d iterations) | %s |\n" %
                        (p["solve_before"]["iters"], fm(p["solve_before"]["ms"], 1.0, 1), p["solve_after"]["iters"], fm(p["solve_after"]["ms"], 1.0, 1)))
                f.write("| device bytes before / after | %d / %d |\n\n" % (p["device_bytes_before"], p["setup_info"]["device_bytes"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
