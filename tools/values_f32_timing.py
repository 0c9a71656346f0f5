#!/usr/bin/env python3
"""What cycle_values = "float32" buys on one MI355X: the problem of the benchmark's variable-coefficient leg -- Q1, kappa(x) smooth,
--cells per direction (default 128 and 192), --levels GMG levels (default 4), CG (rtol 1e-6, maxiter 20, rhs = A u_h(x1 + x2)) around
GMG(Richardson(Jacobi, 10, 2/3) pre = post, V-cycle) -- solved with the option off (the fp64 cycle: the reference of every time
here) and on, by two handles in ONE process, b and x resident in HBM.

  solve     --runs timed runs per leg (default 5), the legs ALTERNATING off / on / off / ..., after --warmup solves each; a run is
            --steps solves (default 5) between two device synchronisations; ms per solve: median, minimum, maximum.  The strict
            criterion: is the SLOWEST run of "on" below the FASTEST run of "off"?
  sweep     per-launch time of the level-0 sweep kernel from the library's HIP events (gmg_profile_enable / gmg_get_kernel_stats,
            event stride 13) in solves of their own, not the timed ones; with the bytes per launch the layout moves
            (layout_bytes: the matrix stream as stored + the row-wise vectors) and the bandwidth that gives, by x-update form
  memory    gmg_device_bytes of both handles, what level_values / level_format / sweep_signature report

    python tools/values_f32_timing.py [--cells 128 192] [--levels 4] [--runs 5] [--steps 5] [--warmup 3]
                                      [--out profiles/values_f32_timing.json] [--md profiles/values_f32_timing.md]
Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), runs=[float(q) for q in v])


def measure(S, po, torch, cells, nlev, a):
    nc = (cells,) * 3
    H = po.build_hierarchy(nc, nlev, 1, kappa=po.smooth_kappa)
    A = H["mats"][0]
    b = A.matvec(po.nodal_values(nc, 1))
    bd = torch.from_numpy(b).cuda()
    n = A.shape[0]
    legs = {}
    for name, cv in (("off", "float64"), ("on", "float32")):
        sm = [S.RichardsonSmoother(S.JacobiLinearSolver(), 10, 2.0 / 3.0)] * (nlev - 1)
        gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sm, post_smoothers=sm,
                                coarsest_solver=S.LUSolver(), maxiter=1, mode="preconditioner", cycle_type="v_cycle", cycle_values=cv)
        solver = S.CGSolver(gmg, maxiter=20, atol=1e-14, rtol=1e-6)
        t0 = time.perf_counter()
        ns = S.numerical_setup(S.symbolic_setup(solver, A), A)
        torch.cuda.synchronize()
        legs[name] = dict(solver=solver, ns=ns, xd=torch.zeros(n, dtype=torch.float64, device="cuda"), setup_s=time.perf_counter() - t0, ms=[])

    def solve(L):
        L["xd"].zero_()
        torch.cuda.synchronize()                              # x0 = 0 is an input: settle it before the solve reads it
        S.solve_(L["xd"], L["ns"], bd)

    for L in legs.values():
        for _ in range(a.warmup):
            solve(L)
    torch.cuda.synchronize()
    for _ in range(a.runs):
        for name in ("off", "on"):
            L = legs[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                solve(L)
            torch.cuda.synchronize()
            L["ms"].append(1e3 * (time.perf_counter() - t0) / a.steps)
    out = dict(cells=cells, levels=nlev, dofs=[int(M.shape[0]) for M in H["mats"]], nnz=[int(M.nnz) for M in H["mats"]], legs={})
    for name, L in legs.items():
        g = L["ns"].P_ns
        g.set_option("prof_stride", 13)
        g.profile(0, True)
        for _ in range(3):
            solve(L)
        torch.cuda.synchronize()
        st = g.kernel_stats()
        g.profile(0, False)
        x = L["xd"].cpu().numpy()
        sweep = dict(launches_timed=int(st["launches"]), avg_us=1e3 * st["total_ms"] / max(st["launches"], 1), layout_bytes=float(st["layout_bytes"]),
                     by_variant={k: dict(launches=v["launches"], avg_us=1e3 * v["avg_ms"], layout_bytes=v["layout_bytes"],
                                         GBps=v["layout_bytes"] / (v["avg_ms"] * 1e-3) / 1e9) for k, v in st["by_variant"].items()})
        sweep["GBps"] = sweep["layout_bytes"] / (sweep["avg_us"] * 1e-6) / 1e9
        out["legs"][name] = dict(ms_per_solve=_stats(L["ms"]), cg_iterations=int(L["solver"].log.num_iters), setup_s=L["setup_s"],
                                 true_rel_residual=float(np.linalg.norm(b - A.matvec(x)) / np.linalg.norm(b)),
                                 sweep_level0=sweep, device_bytes=int(g.device_bytes()),
                                 levels=[dict(g.level_format(l), **g.level_values(l)) for l in range(nlev)],
                                 sweep_signature=g.sweep_signature(0))
    off, on = out["legs"]["off"]["ms_per_solve"], out["legs"]["on"]["ms_per_solve"]
    out["speedup_median"] = off["median"] / on["median"]
    out["strict_criterion_met"] = bool(on["max"] < off["min"])
    out["rel_diff_solutions"] = float(np.linalg.norm(legs["on"]["xd"].cpu().numpy() - legs["off"]["xd"].cpu().numpy())
                                      / np.linalg.norm(legs["off"]["xd"].cpu().numpy()))
    for L in legs.values():
        L["ns"].P_ns.close()
    return out


def markdown(res, a):
    f = lambda s: "%.3f [%.3f .. %.3f]" % (s["median"], s["min"], s["max"])
    lines = ["# `cycle_values = \"float32\"` against the fp64 cycle (`tools/values_f32_timing.py`)", "",
             "One MI355X, one process, two handles; variable-coefficient Q1 (the benchmark's `varcoef` problem), %d levels, CG rtol 1e-6 +"
             " GMG(Jacobi 10/10, omega 2/3).  %d runs of %d solves per leg, the legs alternating, after %d warm-up solves each; ms per"
             " solve as median [min .. max].  The reference of every figure is the option-off leg of the same run." % (a.levels, a.runs, a.steps, a.warmup), "",
             "| cells | dofs | off: ms per solve | on: ms per solve | median ratio | slowest on < fastest off | CG iterations off / on | true residual off / on |",
             "|---|---|---|---|---|---|---|---|"]
    for r in res:
        o, n = r["legs"]["off"], r["legs"]["on"]
        lines.append("| %d^3 | %d | %s | %s | %.3f | %s | %d / %d | %.2e / %.2e |" % (
            r["cells"], r["dofs"][0], f(o["ms_per_solve"]), f(n["ms_per_solve"]), r["speedup_median"], "yes" if r["strict_criterion_met"] else "NO",
            o["cg_iterations"], n["cg_iterations"], o["true_rel_residual"], n["true_rel_residual"]))
    lines += ["", "Level-0 sweep kernel, per launch (HIP events on every 13th launch, in solves of their own), with the bytes the layout moves per launch:", "",
              "| cells | leg | kernel | x-update form | launches timed | us per launch | MB per launch | GB/s |", "|---|---|---|---|---|---|---|---|"]
    for r in res:
        for name in ("off", "on"):
            L = r["legs"][name]
            for k, v in L["sweep_level0"]["by_variant"].items():
                lines.append("| %d^3 | %s | `%s` | %s | %d | %.1f | %.1f | %.0f |" % (r["cells"], name, L["sweep_signature"].split(" ")[0], k, v["launches"],
                                                                                     v["avg_us"], 1e-6 * v["layout_bytes"], v["GBps"]))
    lines += ["", "Device memory and what the handle reports per level (layout, cycle dtype, bytes of cycle stream per stored nonzero):", ""]
    for r in res:
        for name in ("off", "on"):
            L = r["legs"][name]
            lines.append("- %d^3 %s: %.1f MB on the device; %s" % (r["cells"], name, 1e-6 * L["device_bytes"], "; ".join(
                "level %d %s %s %.2f B/nnz" % (l, q["layout"], q["dtype"], q["cycle_stream_bytes_per_nnz"]) for l, q in enumerate(L["levels"]))))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[128, 192])
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    if not torch.cuda.is_available():
        sys.exit("values_f32_timing.py measures on the GPU: no device visible")
    pkg = entry.import_package()
    res = [measure(pkg.solvers, pkg.poisson, torch, c, a.levels, a) for c in a.cells]
    out = dict(runs=a.runs, steps=a.steps, warmup=a.warmup, results=res)
    for path, text in ((a.out, json.dumps(out, indent=1) + "\n"), (a.md, markdown(res, a))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                fh.write(text)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
