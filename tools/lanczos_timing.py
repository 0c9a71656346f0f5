#!/usr/bin/env python3
"""What CG's Lanczos trace costs and what the Lanczos bounds of the ChebyshevSmoother change, on one MI355X, everything in one process,
vectors resident in HBM.

  headline   3-D Poisson Q1 at --cells per direction (default 128), 4 levels, CG + GMG(Jacobi 10/10, omega 2/3), rtol 1e-6 on the
             Dirichlet-lift rhs: ms per solve on a handle that never traced (`never`), with CGSolver(diagnostic=...) (`on`) and with
             the trace switched off again (`off_again`).  `never` is also what a library without the feature runs: --package-dir
             points the tool at another checkout built in place (the parent commit), --only-headline --json-out keep just that
             figure, and --parent-json / --self-json (repeatable) put such runs of the parent and of this tree, with the parent's own
             run-to-run spread, into the report.
  estimator  eig_method power against lanczos, setup seconds, lambda_est per level, iterations and ms per solve, for
               q1      the headline problem with GMG(Chebyshev(Jacobi, 3)), rtol 1e-8
               config3 Q2 at --cells, 5 levels, vertex-star patches, Chebyshev(patch, 4) inside FGMRES(5), rtol 1e-6, as
                       tools/chebyshev_timing.py builds it

The variants alternate inside every round; one warm-up round, then --reps rounds (default 7), each solve between two device
synchronisations; medians, minima and maxima are kept.

    python tools/lanczos_timing.py [--cells 128] [--reps 7] [--package-dir DIR] [--only-headline] [--json-out FILE]
                                   [--parent-json FILE ...] [--self-json FILE ...] [--from-json FILE] [--out profiles/lanczos_timing.md]
Prints one JSON object; writes profiles/lanczos_timing.{json,md} unless --only-headline.  --from-json writes them from a saved
--json-out of this tool and the --parent-json runs, without measuring again (the parent's second run comes after this one's)."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def _fmt(v):
    return "%.3f (%.3f .. %.3f)" % (v["median"], v["min"], v["max"])


def _import(pkg_dir):
    if pkg_dir is None:
        import __graft_entry__ as entry
        return entry.import_package()
    name = "gridapsolvers_jl_amd"
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _finish(out, a):
    """attach the parent runs, write the JSON and the table file"""
    out["parent"] = [json.load(open(p))["headline"]["solve_ms"]["never"] for p in a.parent_json]
    out["self"] = [json.load(open(p))["headline"]["solve_ms"]["never"] for p in a.self_json]
    if a.parent_json:
        out["parent_reps"] = int(json.load(open(a.parent_json[0]))["reps"])
    if a.json_out:
        with open(a.json_out, "w") as f:
            json.dump(out, f, indent=1)
    if not a.only_headline and a.out:
        with open(os.path.splitext(a.out)[0] + ".json", "w") as f:
            json.dump(out, f, indent=1)
        never = out["headline"]["solve_ms"]["never"]
        lines = ["# CG's Lanczos trace and the Lanczos bounds of the ChebyshevSmoother on one MI355X", "",
                 "Written by `tools/lanczos_timing.py`; medians of %d alternating rounds after one warm-up round (min .. max in brackets)." % out["reps"], "",
                 "## headline: Q1 %d^3, 4 levels, CG + GMG(Jacobi 10/10), rtol 1e-6" % out["cells"], "", "dofs per level: %s" % out["headline"]["dofs"], "",
                 "| trace | iterations | ms per solve | against `never` |", "|---|---|---|---|"]
        for k, v in out["headline"]["solve_ms"].items():
            lines.append("| %s | %d | %s | %+.3f ms (%+.2f %%) |" % (k, out["headline"]["iters"][k], _fmt(v), v["median"] - never["median"],
                                                                   100.0 * (v["median"] / never["median"] - 1.0)))
        lines.extend(["", "`never`: no diagnostic; `on`: CGSolver(diagnostic=LanczosDiagnostic(maxiter + 1)), the solve fetches the trace and replays "
                      "it on the host; `off_again`: the same handle after gmg_cg_set_trace(h, 0).  estimate_ of the `on` solve: %.4f." % out["headline"].get("kappa_estimate", float("nan")), ""])
        if out["parent"]:
            pm = [p["median"] for p in out["parent"]]
            sm = [p["median"] for p in out["self"]] or [never["median"]]
            lines.extend(["The parent commit, built from the same tree state, against this tree: `never` alone (all the parent has), every run a "
                          "process of its own (`--only-headline`, %d rounds each), the two libraries in turn:" % out.get("parent_reps", out["reps"]), "", "| run | ms per solve |", "|---|---|"])
            for i in range(max(len(out["parent"]), len(out["self"]))):
                lines.extend("| %s %d | %s |" % (k, i + 1, _fmt(v[i])) for k, v in (("parent", out["parent"]), ("this tree", out["self"])) if i < len(v))
            spread = max(pm) - min(pm) if len(pm) > 1 else float("nan")
            lines.extend(["", "Mean of the medians: parent %.3f ms, this tree %.3f ms, difference %+.3f ms; the parent's own run-to-run spread "
                          "(between its medians) is %.3f ms, and within a run its rounds span up to %.3f ms." %
                          (float(np.mean(pm)), float(np.mean(sm)), float(np.mean(sm) - np.mean(pm)), spread,
                           max(p["max"] - p["min"] for p in out["parent"])), ""])
        for key, title in (("q1", "Q1 %d^3, 4 levels, CG + GMG(Chebyshev(Jacobi, 3)), rtol 1e-8" % out["cells"]),
                           ("config3", "config 3: Q2 %d^3, 5 levels, Chebyshev(patch, 4) inside FGMRES(5), rtol 1e-6" % out["cells"])):
            c = out["estimator"][key]
            lines.extend(["## estimator, " + title, "", "| eig_method | iterations | ms per solve | setup s | lambda_est per level | steps done |", "|---|---|---|---|---|---|"])
            for m in ("power", "lanczos"):
                lines.append("| %s | %d | %s | %.2f | %s | %s |" % (m, c["iters"][m], _fmt(c["solve_ms"][m]), c["setup_s"][m],
                                                                  ", ".join("%.4f" % v for v in c["lambda_est"][m]), c["steps_done"][m]))
            lines.append("")
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--package-dir", default=None, help="the package directory of another checkout, built in place")
    ap.add_argument("--only-headline", action="store_true")
    ap.add_argument("--json-out", default=None)
    ap.add_argument("--parent-json", action="append", default=[])
    ap.add_argument("--self-json", action="append", default=[], help="--only-headline runs of this tree, in processes of their own")
    ap.add_argument("--from-json", default=None, help="no measurement: write the table file from a saved --json-out and the --parent-json runs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lanczos_timing.md"))
    a = ap.parse_args()
    if a.from_json:
        out = json.load(open(a.from_json))
        _finish(out, a)
        print(json.dumps(out))
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("lanczos_timing.py measures on the GPU: no device visible")
    pkg = _import(a.package_dir)
    S, po = pkg.solvers, pkg.poisson
    has_trace = hasattr(S, "LanczosDiagnostic")

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

    out = dict(reps=a.reps, cells=a.cells)
    # ---------------------------------------------------------------- headline
    nc, nlev = (a.cells,) * 3, 4
    H = po.build_hierarchy(nc, nlev, 1)
    A = H["mats"][0]
    bd = torch.from_numpy(po.dirichlet_lift_rhs(nc, 1)).cuda()
    xd = torch.zeros_like(bd)
    kw = dict(maxiter=20, atol=1e-14, rtol=1e-6)

    def cg_gmg(sm, diag=None, **kws):
        gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sm, post_smoothers=sm, maxiter=1)
        solver = S.CGSolver(gmg, diagnostic=diag, **kws) if diag is not None else S.CGSolver(gmg, **kws)
        t0 = time.perf_counter()
        ns = S.numerical_setup(S.symbolic_setup(solver, A), A)
        torch.cuda.synchronize()
        return ns, solver, time.perf_counter() - t0

    def solve_fn(ns, x, b):
        def fn():
            x.zero_()
            S.solve_(x, ns, b)
        return fn

    jac = [S.RichardsonSmoother(S.JacobiLinearSolver(), 10, 2.0 / 3.0)] * (nlev - 1)
    handles = {"never": cg_gmg(jac, **kw)}
    if has_trace and not a.only_headline:
        handles["on"] = cg_gmg(jac, S.LanczosDiagnostic(kw["maxiter"] + 1), **kw)
        handles["off_again"] = cg_gmg(jac, S.LanczosDiagnostic(kw["maxiter"] + 1), **kw)
        handles["off_again"][0].P_ns.cg_set_trace(0)
        handles["off_again"][1].diag = None
    hd = dict(dofs=[int(M.shape[0]) for M in H["mats"]])
    hd["solve_ms"] = alternate({k: solve_fn(v[0], xd, bd) for k, v in handles.items()})
    hd["iters"] = {k: int(v[1].log.num_iters) for k, v in handles.items()}
    if "on" in handles:
        hd["kappa_estimate"] = float(S.estimate_(handles["on"][1].diag))
    for ns, _s, _t in handles.values():
        ns.P_ns.close()
    out["headline"] = hd
    # ---------------------------------------------------------------- estimator
    if not a.only_headline:
        est = {}
        kw8 = dict(maxiter=30, atol=1e-14, rtol=1e-8)
        q1, handles = dict(setup_s={}, lambda_est={}, steps_done={}, iters={}), {}
        for m in ("power", "lanczos"):
            sm = [S.ChebyshevSmoother(S.JacobiLinearSolver(), 3, eig_method=m) for _ in range(nlev - 1)]
            handles[m] = cg_gmg(sm, **kw8)
            q1["setup_s"][m] = handles[m][2]
            infos = [handles[m][0].P_ns.chebyshev_info(l) for l in range(nlev - 1)]
            q1["lambda_est"][m] = [i["lambda_est"] for i in infos]
            q1["steps_done"][m] = [i["eig_steps_done"] for i in infos]
        q1["solve_ms"] = alternate({k: solve_fn(v[0], xd, bd) for k, v in handles.items()})
        for k, (ns, solver, _t) in handles.items():
            q1["iters"][k] = int(solver.log.num_iters)
            ns.P_ns.close()
        est["q1"] = q1
        nl3, order = 5, 2
        H3 = po.build_hierarchy(nc, nl3, order, stream_min_rows=1000000)
        b3 = torch.from_numpy(po.dirichlet_lift_rhs(nc, order)).cuda()
        x3 = torch.zeros_like(b3)
        Ms = [S.PatchSolver(*po.vertex_star_patches(H3["ncells"][l], order)) for l in range(nl3 - 1)]
        c3, handles = dict(dofs=[int(M.shape[0]) for M in H3["mats"]], setup_s={}, lambda_est={}, steps_done={}, iters={}), {}
        for m in ("power", "lanczos"):
            sm = [S.ChebyshevSmoother(M, 4, eig_method=m) for M in Ms]
            gmg = S.GMGLinearSolver(H3["mats"], H3["prolongations"], H3["restrictions"], pre_smoothers=sm, post_smoothers=sm, maxiter=1)
            solver = S.FGMRESSolver(5, gmg, maxiter=20, atol=1e-14, rtol=1e-6)
            t0 = time.perf_counter()
            ns = S.numerical_setup(S.symbolic_setup(solver, H3["mats"][0]), H3["mats"][0])
            torch.cuda.synchronize()
            c3["setup_s"][m] = time.perf_counter() - t0
            infos = [ns.P_ns.chebyshev_info(l) for l in range(nl3 - 1)]
            c3["lambda_est"][m] = [i["lambda_est"] for i in infos]
            c3["steps_done"][m] = [i["eig_steps_done"] for i in infos]
            handles[m] = (ns, solver)
        c3["solve_ms"] = alternate({k: solve_fn(v[0], x3, b3) for k, v in handles.items()})
        for k, (ns, solver) in handles.items():
            c3["iters"][k] = int(solver.log.num_iters)
            ns.P_ns.close()
        est["config3"] = c3
        out["estimator"] = est
    _finish(out, a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
