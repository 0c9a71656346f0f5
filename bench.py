#!/usr/bin/env python3
"""bench.py -- DoFs/s of CG + GMG V-cycle on 3-D Poisson Q1 (BASELINE.json metric).

A "step" is one complete `solve!(x, CGNumericalSetup, b)` (Krylov/CGSolvers.jl:73-120 with the GMG V-cycle
preconditioner GMGLinearSolvers.jl:468-502,612-645) from x = 0 to rtol, inputs resident in HBM.

The JSON line has the SAME shape at every --gpus N (key <-> leg):
    value, ms_per_step, roofline_compressed   default leg: the product as shipped, gmg_setup picks the storage layout
                                              (row-pattern dictionary on this constant-coefficient operator)
    value_generic, ms_per_step_generic,       generic leg: every structure-exploiting layout off -- the 12 B/nnz (col,val)
    roofline                                  stream SURVEY 8(d)'s byte model is written for
    cpu_baseline                              the CPU oracle (oracle/, a cited port of the reference algorithm) on the host cores
N = 1  BASELINE configs[1]: 128^3 cells, Q1, 4 levels, Richardson(Jacobi,10,2/3) pre = post, exact coarse solve,
       CG(maxiter=20, atol=1e-14, rtol=1e-6), rhs = the reference test problem u = x1 + x2
       (test/LinearSolvers/GMGTests.jl:52,109-124,204-213).  Further legs of a --full run:
         variable_coefficient   kappa(x) grad u . grad v: every row's values distinct (SELL-O: 8 B/nnz)
         weak_scaling_ref       the per-GPU problem of the N > 1 runs (288^3, 6 levels) on this one GPU; its value is also the
                                top-level `weak_anchor_value` -- what value / N of an N > 1 line is to be held against
         host_io                the same solves with b / x as HOST arrays through GMG_MEM_HOST -- what the Julia binding passes --
                                pageable, page-locked once (gmg_host_register) and with the x0_zero option; + one V-cycle per call
                                (`precond_only`: the library as the preconditioner of a host-language Krylov loop)
         config3                BASELINE configs[2] at its stated size: Q2 256^3, 5 levels, vertex-star patch smoother
                                Richardson(PatchSolver,10,0.2), FGMRES(5) (test/LinearSolvers/GMGTests.jl:18-47,119-123)
         config5                BASELINE configs[4] on one GPU: 2-D Stokes Q2 / P1disc (lid-driven cavity), FGMRES(20) with the upper
                                block-triangular preconditioner, GMG(patch smoothers, patch-corrected prolongation) on the velocity
                                block, CG-Jacobi on the pressure block (test/Applications/StokesGMG.jl:79-166)
N > 1  BASELINE configs[3]: 288^3 cells per GPU (576^3 on 2x2x2), 6 levels, box row partition, halo exchange and
       scalar all-reduces over RCCL; launched by torch.distributed.run, or by bench.py itself when WORLD_SIZE is unset.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR]
                    [--full [--legs default,generic,varcoef,weak_ref,host_io,config3,config5,rccl_loopback,cpu]]
                    [--allow-degraded]   (N > 1 only: without it a run whose transport is not RCCL on all N ranks exits non-zero)

A plain run sets up the default leg, warms up, times the steps and prints the line: nothing else.  --full adds everything beyond
the headline figure: the further legs (all of them unless --legs / --no-* pick), the CPU baseline and the oracle checks, the
default leg's per-level sweep profiles, the streaming-ceiling probes and its l2 error.

         rccl_loopback          functional: the 2x2x2 partition of a Q1 problem folded onto this GPU, solved through the product's halo
                                exchange and all-reduces over RCCL (one real rank, self messages); bitwise against the host transport

Prints ONE JSON line (rank 0) of <= 4 KB -- value, ms_per_step and roofline all describe the default leg.  Everything else the run
measured goes to GMG_BENCH_DETAILS=<file> if set, and a --full run without it writes profiles/bench_legs_latest.json."""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec, /opt/skills/guides/MI355X_MICROARCH.md
WS_CELLS, WS_LEVELS = 288, 6   # per-GPU problem of the N > 1 runs: BASELINE configs[3] = 576^3 cells on 2x2x2 GPUs, 6 levels
# the generic (12 B/nnz) leg: per-handle options (gmg_set_option), not environment variables
GENERIC_OPTIONS = {"vdict": 0, "idx16": 0, "pattern": 0, "opattern": 0}


def prof_stride_for(steps, sweeps_per_solve=60):
    """how rarely the timed solves' sweep launches are bracketed by HIP events: the largest odd stride that leaves >= 8 samples"""
    env = os.environ.get("GMG_PROF_STRIDE")
    if env:
        return int(env)
    for s in (61, 31, 13, 7):
        if steps * sweeps_per_solve // s >= 8:
            return s
    return 7
ALL_LEGS = ("default", "generic", "varcoef", "weak_ref", "host_io", "config3", "config5", "rccl_loopback", "cpu")
LEGS_NOTE = ("same key <-> leg mapping at every --gpus N: default leg (the product as shipped: gmg_setup picks the storage layout) = `value`, "
             "`ms_per_step`, `roofline_compressed`; generic leg (every structure-exploiting layout off: the 12 B/nnz (col,val) stream SURVEY 8(d)'s "
             "byte model describes) = `value_generic`, `ms_per_step_generic`, `roofline`.  N = 1 runs BASELINE configs[1] (128^3) and carries the "
             "per-GPU problem of the N > 1 runs on one GPU as `weak_anchor_value` / `weak_scaling_ref`; N > 1 runs 288^3 cells per GPU: hold "
             "value / N against weak_anchor_value, never against the N = 1 `value`.  Further N = 1 legs: variable_coefficient, host_io "
             "(`value_host_io`: b / x as host arrays through GMG_MEM_HOST, the Julia binding's path), config3 (Q2 + patch smoother + FGMRES).")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=None, help="cells per direction per GPU (default: 128 at N=1, 288 at N>1)")
    ap.add_argument("--levels", type=int, default=None, help="GMG levels (default: 4 at N=1, 6 at N>1)")
    ap.add_argument("--full", action="store_true",
                    help="run everything beyond the headline figure too: the further legs (--legs, --no-*), the CPU baseline and oracle checks, "
                         "the per-level sweep profiles, the streaming-ceiling probes, the l2 error and the details file in profiles/")
    ap.add_argument("--legs", default="all", help="with --full: comma list of " + ",".join(ALL_LEGS) + " (default: all; `default` always runs)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-varcoef", action="store_true", help="skip the variable-coefficient leg")
    ap.add_argument("--no-weak-ref", action="store_true", help="skip the weak-scaling reference leg (the N > 1 per-GPU problem on one GPU)")
    ap.add_argument("--no-generic", action="store_true", help="skip the generic (12 B/nnz) leg")
    ap.add_argument("--no-host-io", action="store_true", help="skip the host-vector leg")
    ap.add_argument("--no-config3", action="store_true", help="skip the config-3 leg (Q2, patch smoother, FGMRES)")
    ap.add_argument("--config3-cells", type=int, default=256, help="cells per direction of the config-3 leg (BASELINE configs[2]: 256; 5 levels)")
    ap.add_argument("--config3-levels", type=int, default=5)
    ap.add_argument("--no-config5", action="store_true", help="skip the config-5 leg (Stokes Q2/P1disc, block-triangular FGMRES)")
    ap.add_argument("--config5-cells", type=int, default=1024, help="cells per direction of the 2-D Stokes leg (2 (2n-1)^2 velocity dofs; 1024: 8.4e6 -- one "
                                                                     "vector of the finest velocity level is 67 MB, a sweep's operands outgrow the 256 MB Infinity Cache)")
    ap.add_argument("--config5-levels", type=int, default=7)
    ap.add_argument("--config5-cpu-cells", type=int, default=256, help="size of the config-5 oracle check / CPU baseline (the oracle's patch solves are sequential)")
    ap.add_argument("--config5-cpu-levels", type=int, default=5)
    ap.add_argument("--loopback-cells", type=int, default=48, help="cells per direction per (virtual) rank of the rccl_loopback leg")
    ap.add_argument("--loopback-levels", type=int, default=4)
    ap.add_argument("--allow-degraded", action="store_true",
                    help="N > 1: accept the host-staged transport / in-stream exchanges when RCCL is unavailable (the line then says degraded: true)")
    ap.add_argument("--rhs", choices=["lin", "rand"], default="lin")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the headline leg's last timed solve returned (solution x, residual history) "
                         "as DIR/<name>.npy (float64, <= 64 MB in all: a seeded sample of x beyond that)")
    args = ap.parse_args()
    if args.cells is None:
        args.cells = 128 if args.gpus == 1 else WS_CELLS
    if args.levels is None:
        args.levels = 4 if args.gpus == 1 else WS_LEVELS
    legs = set(ALL_LEGS) if args.legs == "all" else set(x.strip() for x in args.legs.split(",") if x.strip())
    bad = legs - set(ALL_LEGS)
    if bad:
        raise SystemExit(f"unknown legs {sorted(bad)}; choose from {ALL_LEGS}")
    for flag, leg in (("no_cpu_baseline", "cpu"), ("no_varcoef", "varcoef"), ("no_weak_ref", "weak_ref"), ("no_generic", "generic"),
                      ("no_host_io", "host_io"), ("no_config3", "config3"), ("no_config5", "config5")):
        if getattr(args, flag):
            legs.discard(leg)
    if not args.full:
        # a plain run times the headline leg and nothing else; the --no-* flags have nothing left to drop
        if args.legs != "all" and legs - {"default"}:
            raise SystemExit(f"--legs {args.legs}: the legs beyond `default` run with --full only")
        legs = set()
    legs.add("default")
    args.legset = legs
    args.no_generic = "generic" not in legs          # (multigpu.run_bench reads this)
    return args


# ---------------------------------------------------------------------------------------------------------
# N > 1 without a launcher: start one worker per GPU ourselves (before this process touches a GPU)
# ---------------------------------------------------------------------------------------------------------
def self_launch(args):
    import torch
    ndev = torch.cuda.device_count()           # counting devices does not initialise the GPU
    if ndev < args.gpus and not os.environ.get("GMG_SHARE_GPU"):
        raise SystemExit(f"bench.py --gpus {args.gpus}: only {ndev} GPU(s) visible")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.exit(subprocess.call(cmd, env=env))      # child processes; this one never initialises a GPU


# ---------------------------------------------------------------------------------------------------------
# cpu_baseline: oracle/cpu_baseline.py in a child process (own OpenMP runtime, pinned threads, no GPU)
# ---------------------------------------------------------------------------------------------------------
def usable_cores():
    n = len(os.sched_getaffinity(0))
    quota = None
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = float(q) / float(p)
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / p
        except Exception:
            pass
    return n, quota, (n if quota is None else max(1, min(n, int(quota + 0.5))))


def run_oracle_child(cells, levels, rhs, kappa, variant, threads, limit_s, max_reps, want_x, config3=False):
    env = dict(os.environ)
    for k in list(env):
        if k.startswith(("OMP_", "GOMP_", "KMP_")):
            del env[k]
    env["OMP_NUM_THREADS"] = str(threads)
    if variant == "omp":
        env["OMP_PROC_BIND"] = "close"
        env["OMP_PLACES"] = "cores"
    xfile = None
    cmd = [sys.executable, os.path.join(ROOT, "oracle", "cpu_baseline.py"), "--cells", str(cells), "--levels", str(levels),
           "--rhs", rhs, "--kappa", kappa, "--variant", variant, "--limit-s", str(limit_s), "--max-reps", str(max_reps)]
    if config3:
        cmd.append("--config3")
    if want_x:
        fd, xfile = tempfile.mkstemp(suffix=".npy")
        os.close(fd)
        cmd += ["--out-x", xfile]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError(f"oracle child failed: {p.stderr[-400:]}")
    out = json.loads(p.stdout.strip().splitlines()[-1])
    x = None
    if xfile:
        x = np.load(xfile)
        os.unlink(xfile)
    return out, x


def cpu_baseline(cells, levels, rhs, config3=False, limit_seq=10.0, limit_omp=8.0):
    """kind "port": oracle/gmg_oracle.c (same operation sequence as the reference) on full solves of the workload,
    bounded to ~10 s per variant.  (1) one thread -- the analogue of ONE reference MPI rank, also what the GPU result is
    checked against; (2) all usable host cores (OpenMP build of the same file, pinned threads, parallel first touch) -- the
    analogue of the reference under MPI on P ranks.  `value` is the faster of the two, `cores` says which."""
    naff, quota, ncore = usable_cores()
    what = "FGMRES(5)+GMG(patch smoother)" if config3 else "CG+GMG"
    r1, x = run_oracle_child(cells, levels, rhs, "const", "seq", 1, limit_seq, 8, True, config3)
    n = r1["dofs"]
    out = dict(value=n / r1["seconds"], unit="DoFs/s", cores=1, kind="port",
               sample=f"{r1['reps']} full {what} solves ({n} dofs, {r1['iters']} iterations each) by "
                      f"oracle/gmg_oracle.c in a child process, single thread, {r1['seconds']:.2f} s per solve",
               iters=r1["iters"], seconds=r1["seconds"], single_thread_value=n / r1["seconds"],
               host=dict(affinity_cores=naff, cgroup_cpu_quota=quota, usable_cores=ncore, os_cpu_count=os.cpu_count()))
    if ncore > 1 and not config3:
        try:
            rp, _ = run_oracle_child(cells, levels, rhs, "const", "omp", ncore, limit_omp, 16, False, config3)
            out["all_cores"] = dict(value=n / rp["seconds"], cores=rp["threads"], seconds=rp["seconds"], iters=rp["iters"],
                                    reps=rp["reps"], speedup_vs_single_thread=r1["seconds"] / rp["seconds"], omp_env=rp["omp_env"])
            if rp["iters"] == r1["iters"] and rp["seconds"] < r1["seconds"]:
                out.update(value=n / rp["seconds"], cores=rp["threads"], seconds=rp["seconds"],
                           sample=f"{rp['reps']} full {what} solves ({n} dofs, {rp['iters']} iterations each) by "
                                  f"the OpenMP build of oracle/gmg_oracle.c on {rp['threads']} pinned host threads (child process, "
                                  f"parallel first touch), {rp['seconds']:.3f} s per solve; single thread: {r1['seconds']:.2f} s per solve")
        except Exception as e:      # the OpenMP build is optional
            out["all_cores"] = {"error": str(e)[-300:]}
    elif config3:
        out["all_cores"] = {"skipped": "the oracle's patch solve is sequential (PatchSolvers.jl:279-300 is a serial loop over patches)"}
    else:
        out["all_cores"] = {"skipped": f"process may use {ncore} core (affinity {naff}, cgroup quota {quota})"}
    return out, x, r1["iters"], np.asarray(r1["hist"])


# ---------------------------------------------------------------------------------------------------------
def kernel_label(fmt):
    """name of the finest-level fused sweep kernel for the storage layout the setup chose"""
    what = "<EPI_SWEEP,ONEG> (fused Richardson-Jacobi sweep, finest level, " + fmt["layout"]
    if fmt["row_patterns"]:
        return "sells_*sweep_kernel (fused Richardson-Jacobi sweep, finest level, " + fmt["layout"] + \
               ": row-pattern dictionary in LDS, %.2f B/nnz of matrix stream)" % fmt["stream_bytes_per_nnz"]
    if fmt["value_dictionary"] or fmt["idx16"]:
        return "sellc_kernel" + what + ", lossless stream compression %.0f B/nnz)" % fmt["stream_bytes_per_nnz"]
    if fmt["layout"] == "SELL-O":
        return "sello_kernel" + what + ": 8 B/nnz value stream, column offsets from an offset-pattern table in LDS)"
    if fmt["layout"] == "SELL-64":
        return "sell_kernel" + what + ", plain 12 B/nnz (col,val) stream)"
    return "csr_stream1_kernel" + what + ")"


def kernel_family(fmt):
    if fmt["row_patterns"]:
        return "sells_kernel"
    if fmt["value_dictionary"] or fmt["idx16"]:
        return "sellc_kernel"
    return {"SELL-64": "sell_kernel", "SELL-O": "sello_kernel"}.get(fmt["layout"], "csr_stream1_kernel")


def kernel_source_sha():
    """sha256 of the kernel source the counters were / are measured on (csrc/kernels.hpp)"""
    import hashlib
    return hashlib.sha256(open(os.path.join(ROOT, "gridapsolvers.jl_amd", "csrc", "kernels.hpp"), "rb").read()).hexdigest()[:16]


def committed_traffic(family, cells, levels, rows, signature, order=1):
    """HBM bytes per launch of the timed kernel from the committed PMC passes (profiles/traffic_latest.json, written by
    profiles/summarize.py from separate `rocprofv3 --pmc FETCH_SIZE` / `WRITE_SIZE` runs of THIS command).  Counters cannot
    be read from inside the bench process, so the figure is only attached when the profiled run matches the current one in
    kernel family, problem, row count, the sweep's signature as the library reports it (gmg_sweep_signature: template
    arguments + launch geometry) AND the sha of csrc/kernels.hpp; otherwise null, with the reason."""
    tfile = os.path.join(ROOT, "profiles", "traffic_latest.json")
    try:
        T = json.load(open(tfile))
    except Exception:
        return None, "no profiles/traffic_latest.json"
    if T.get("kernels_hpp_sha") != kernel_source_sha():
        return None, f"profiles/traffic_latest.json ({T.get('tag', '?')}) was measured on another version of csrc/kernels.hpp: not attached"
    for rec in T.get("kernels", []):
        if rec.get("family") == family and rec.get("cells") == cells and rec.get("levels") == levels and rec.get("rows") == rows \
                and rec.get("order", 1) == order:
            if signature is not None and rec.get("signature") != signature:
                return None, f"profiled sweep was '{rec.get('signature')}', this run's is '{signature}': not attached"
            return rec.get("hbm_bytes_per_launch"), f"profiles/traffic_latest.json ({T.get('tag', '?')}: rocprofv3 --pmc passes of the same command, same " \
                                                      f"kernel source and sweep signature; not re-measured in this run)"
    return None, "no matching record in profiles/traffic_latest.json"


def pcie_probe(torch, nbytes):
    """page-locked host <-> device copy rates of this box (GB/s), the ceiling of every host-vector figure"""
    n = nbytes // 8
    hp = torch.empty(n, dtype=torch.float64).pin_memory()
    d = torch.empty(n, dtype=torch.float64, device="cuda")
    out = {}
    for name, dst, src in (("h2d", d, hp), ("d2h", hp, d)):
        dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        out[name + "_GBs"] = 5 * nbytes / (time.perf_counter() - t0) / 1e9
    del hp, d
    return out


def host_io_leg(torch, S, ns, b, dev_ms, steps, label):
    """The solves of a leg again with b / x as HOST arrays through GMG_MEM_HOST -- exactly what julia/GridapSolversAMD.jl passes for
    Vector{Float64} -- timed per call (the call returns when x is back in the caller's array).  Variants: pageable arrays (the
    library pipelines them through its own page-locked chunks), the same arrays page-locked ONCE with gmg_host_register (the pattern
    of ext/GridapPETScExt/PETScCaches.jl:23-36), and additionally the x0_zero option (the initial guess is not uploaded).
    precond_only: ONE V-cycle per call with host r / z (gmg_apply) -- the library as preconditioner of a host-language Krylov loop."""
    g = ns.P_ns
    n = b.size
    nb = 8 * n

    def timed(fn, before, reps, warm=1):
        ts = []
        for i in range(warm + reps):
            if before:
                before()                          # the caller's own work (fill!(x, 0.0)): not part of solve!
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if i >= warm:
                ts.append(dt)
        return float(np.mean(ts)), float(np.min(ts))

    def solve_on(x, bb):
        return (lambda: S.solve_(x, ns, bb)), (lambda: x.fill(0.0))
    out = {"workload": label, "bytes_per_vector": nb, "device_resident_ms": dev_ms, "pcie": pcie_probe(torch, nb)}
    reps = max(3, steps // 2)
    b1, x1 = b.copy(), np.zeros(n)
    m, mn = timed(*solve_on(x1, b1), reps)
    out["pageable"] = dict(ms_per_step=m * 1e3, min_ms=mn * 1e3, value=n / m)
    xp = x1.copy()
    b2, x2 = b.copy(), np.zeros(n)
    t0 = time.perf_counter()
    g.pin(b2, x2)
    out["register_ms_once"] = (time.perf_counter() - t0) * 1e3
    m, mn = timed(*solve_on(x2, b2), reps)
    out["registered"] = dict(ms_per_step=m * 1e3, min_ms=mn * 1e3, value=n / m)
    g.set_option("x0_zero", 1)
    m, mn = timed(*solve_on(x2, b2), reps)
    g.set_option("x0_zero", 0)
    out["registered_x0_zero"] = dict(ms_per_step=m * 1e3, min_ms=mn * 1e3, value=n / m)
    out["bitwise_equal_pageable_vs_registered"] = bool(np.array_equal(xp, x2))
    # floor of this path on this box: the device-resident solve + b up + x down at the measured link rates
    up, down = out["pcie"]["h2d_GBs"], out["pcie"]["d2h_GBs"]
    floor_ms = dev_ms + nb / up / 1e6 + nb / down / 1e6
    out["floor_ms"] = floor_ms
    out["floor_note"] = ("device-resident solve + 8N bytes up (b) + 8N bytes down (x) at the page-locked copy rates measured in this run; "
                         "x only exists after the last CG update and b is needed by the first sweep, so neither copy can hide behind the solve")
    out["value"] = out["registered_x0_zero"]["value"]
    out["ms_per_step"] = out["registered_x0_zero"]["ms_per_step"]
    out["frac_of_device_resident"] = dev_ms / out["ms_per_step"]
    out["frac_of_floor"] = floor_ms / out["ms_per_step"]
    # one V-cycle per call (GMG as :preconditioner, maxiter = 1): z = M r with host vectors vs device vectors
    r_h, z_h = b2, x2
    m_h, _ = timed(lambda: S.solve_(z_h, g, r_h), None, reps)
    rd, zd = torch.from_numpy(b).cuda(), torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def dev_call():
        S.solve_(zd, g, rd)
        torch.cuda.synchronize()
    m_d, _ = timed(dev_call, None, reps)
    out["precond_only"] = dict(host_registered_ms=m_h * 1e3, device_ms=m_d * 1e3, frac=m_d / m_h,
                               note="one gmg_apply (one V-cycle) per call: 16 N bytes over PCIe per application -- a host-language Krylov loop "
                                    "should hand the library device vectors or call the whole-solve entry points (gmg_cg_solve / gmg_fgmres_solve)")
    out["host_io_stats"] = g.host_io_stats()
    return out


LINE_LIMIT = 4096          # bytes: round 5's 22.7 KB line was more than the driver's parser takes
_REAL_STDOUT = None        # the process's original stdout, see claim_stdout()


def claim_stdout():
    """From here on ONLY the JSON line reaches the process's real stdout: file descriptor 1 is pointed at stderr and the line is written
    to a duplicate of the original.  RCCL prints a version banner to stdout when NCCL_DEBUG=VERSION is set (it is, on the GPU boxes) --
    through C stdio, i.e. at process EXIT when stdout is a pipe or a file: five lines BEHIND the JSON line of any run that initialises a
    communicator (every N > 1 run; the rccl_loopback leg at N = 1)."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.dup(1)
        os.dup2(2, 1)


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None}


def _short(s, n):
    s = str(s)
    return s if len(s) <= n else s[: n - 3] + "..."


def emit(out, full_run):
    """Rank 0: write EVERYTHING this run measured (all legs, notes, per-level and per-form tables) to profiles/bench_legs_latest.json (and a
    copy under gpurun_out/, the directory gpurun brings back), then print ONE line of <= 4 KB whose value / ms_per_step / roofline all
    describe the SAME leg -- the default leg: the product as shipped, storage layout chosen by gmg_setup.  Its roofline prices the dominant
    kernel with the bytes that layout moves per launch (every operand once, no cache credit) next to the PMC-measured HBM traffic; the
    generic leg (the 12 B/nnz stream SURVEY 8(d)'s model is written for) rides along as one small object of its own.
    A plain run (no --full) writes the details only where GMG_BENCH_DETAILS points."""
    full = dict(out)
    rc, rg = full.pop("roofline_compressed", None), full.pop("roofline", None)
    compressed = bool(rc) and rc.get("speedup_vs_12B_per_nnz_model", 2.0) > 1.0 + 1e-9
    head = rc if (compressed or not (isinstance(rg, dict) and rg.get("achieved"))) else rg     # no structure found: the default leg IS the generic stream
    full["roofline"], full["roofline_generic"] = head, rg
    paths = []
    # GMG_BENCH_DETAILS=<file>: the details go there and nowhere else (tests: keeps the tracked profiles/ copy out of their way)
    targets = [os.environ["GMG_BENCH_DETAILS"]] if os.environ.get("GMG_BENCH_DETAILS") else \
        [os.path.join(ROOT, d, "bench_legs_latest.json") for d in ("profiles", "gpurun_out")]
    if not full_run and not os.environ.get("GMG_BENCH_DETAILS"):
        targets = []
    for t in targets:
        try:
            os.makedirs(os.path.dirname(t) or ".", exist_ok=True)
            with open(t, "w") as f:
                json.dump(full, f, indent=1, default=float)
            paths.append(os.path.relpath(t, ROOT) if t.startswith(ROOT) else t)
        except OSError:
            pass
    line = _pick(full, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                        "dtype", "data", "rccl_ranks", "weak_anchor_value"))
    for k in ("vs_baseline", "weak_anchor_value"):
        line.setdefault(k, None)
    cfg = _pick(full.get("config", {}), ("workload", "dofs", "dofs_per_gpu", "nnz", "levels", "cg_iterations", "iterations_match_cpu",
                                         "rel_diff_vs_cpu_solution", "transport", "degraded", "halo_exchanges_per_solve", "allreduces_per_solve"))
    cfg["workload"] = _short(cfg.get("workload", ""), 420)
    line["config"] = cfg
    r = _pick(head or {}, ("bound", "kernel", "bytes_model", "bytes_per_launch", "avg_launch_ms", "launches_timed", "achieved", "peak", "unit",
                           "frac", "traffic", "traffic_GBs"))
    for k in ("traffic",):
        r.setdefault(k, None)
    r["kernel"], r["bytes_model"] = _short(r.get("kernel", ""), 200), _short(r.get("bytes_model", ""), 260)
    r["leg"] = "default (same leg as value / ms_per_step)"
    line["roofline"] = r
    if isinstance(rg, dict) and rg is not head and rg.get("achieved"):
        line["generic_leg"] = dict(value=full.get("value_generic"), ms_per_step=full.get("ms_per_step_generic"),
                                   what="same problem, every structure-exploiting layout off: the 12 B/nnz (col,val) stream of SURVEY 8(d)",
                                   roofline=_pick(rg, ("bytes_per_launch", "avg_launch_ms", "launches_timed", "achieved", "frac", "traffic", "traffic_GBs")))
    lb = full.get("rccl_loopback")
    if isinstance(lb, dict):
        line["rccl_loopback"] = _pick(lb, ("rccl_ranks", "virtual_ranks", "exchanges_per_solve", "allreduces_per_solve", "bitwise_equal_host_transport",
                                           "ms_per_step_overlapped", "ms_per_step_unpartitioned", "error"))
    cb = full.get("cpu_baseline")
    if isinstance(cb, dict):
        c = _pick(cb, ("value", "unit", "cores", "kind", "seconds", "single_thread_value", "error"))
        c["sample"] = _short(cb.get("sample", ""), 300)
        line["cpu_baseline"] = c
    line["details"] = paths[0] if paths else None
    txt = json.dumps(line, default=float)
    if len(txt) > LINE_LIMIT:                    # never again a line the driver cannot take: drop the optional parts first
        for k in ("generic_leg", "rccl_loopback", "details"):
            line.pop(k, None)
        line["config"]["workload"] = _short(line["config"]["workload"], 160)
        txt = json.dumps(line, default=float)
    assert len(txt) <= LINE_LIMIT, len(txt)
    json.loads(txt)
    sys.stdout.flush()
    os.write(_REAL_STDOUT if _REAL_STDOUT is not None else 1, (txt + "\n").encode())


DUMP_LIMIT = 64 << 20      # bytes, all --dump-outputs files together


def dump_outputs(dirname, x, residuals):
    """--dump-outputs: the arrays a caller of the timed solve receives -- x and the residual history (float64).  An x larger than the
    budget is written as a fixed, seeded sample x[idx] with its indices (x_index.npy, exact in float64), the same on every run."""
    os.makedirs(dirname, exist_ok=True)
    x = np.ascontiguousarray(x, dtype=np.float64)
    res = np.ascontiguousarray(residuals, dtype=np.float64)
    arrays = {"residuals": res}
    room = (DUMP_LIMIT - res.nbytes - 3 * 4096) // 8            # (4 KB per .npy header, generously)
    if x.size <= room:
        arrays["x"] = x
    else:
        idx = np.sort(np.random.default_rng(20240601).choice(x.size, size=room // 2, replace=False))
        arrays["x"], arrays["x_index"] = x[idx], idx.astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


def main():
    args = parse()
    if args.dump_outputs and args.gpus > 1:
        raise SystemExit("--dump-outputs: single-GPU runs only (--gpus 1)")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)
    claim_stdout()
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    assert torch.cuda.is_available(), "bench.py needs a GPU (the product has no CPU path)"
    if os.environ.get("GMG_SHARE_GPU"):          # test hook: several ranks on one GPU (host transport only)
        local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    if world > 1:
        if os.environ.get("GMG_TRANSPORT", "rccl") == "host":
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    pkg = entry.import_package()
    po, S = pkg.poisson, pkg.solvers
    legs = args.legset

    def make_solver(H, nlev, maxiter, atol, rtol, options=None):
        sm = [S.RichardsonSmoother(S.JacobiLinearSolver(), 10, 2.0 / 3.0)] * (nlev - 1)
        gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sm, post_smoothers=sm,
                                coarsest_solver=S.LUSolver(), maxiter=1, mode="preconditioner", cycle_type="v_cycle", options=options)
        return S.CGSolver(gmg, maxiter=maxiter, atol=atol, rtol=rtol)

    maxiter, atol, rtol = (20, 1e-14, 1e-6) if args.rhs == "lin" else (100, 1e-14, 1e-8)

    def leg(H, b, nlev, steps, warmup, options=None):
        """numerical_setup + `steps` timed solves; HIP events around every prof_stride-th finest-level sweep launch of the timed solves
        (the roofline's per-launch time).  Every sampled launch costs the stream ~11 us (two event bubbles): at the library's default
        stride of 7 that was 5 % of the 128^3 solve time this function reports, so the stride is the largest of 61 / 31 / 13 / 7 that
        still leaves >= 8 samples (60 finest sweeps per solve; odd and coprime with 60: both alternating sweep forms, every position)."""
        solver = make_solver(H, nlev, maxiter, atol, rtol, options)
        t0 = time.perf_counter()
        ns = S.numerical_setup(S.symbolic_setup(solver, H["mats"][0]), H["mats"][0])
        t_setup = time.perf_counter() - t0
        n = H["mats"][0].shape[0]
        bd = torch.from_numpy(b).cuda()
        xd = torch.zeros(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def step():
            xd.zero_()
            torch.cuda.synchronize()          # x0 = 0 is an input: settle it before the solve reads it
            S.solve_(xd, ns, bd)
        for _ in range(warmup):
            step()
        stride = prof_stride_for(steps)
        ns.P_ns.set_option("prof_stride", stride)
        ns.P_ns.profile(0, True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st = ns.P_ns.kernel_stats()
        st["prof_stride"] = stride
        ns.P_ns.profile(0, False)
        fmt = ns.P_ns.level_format(0)
        fmt["sweep_signature"] = ns.P_ns.sweep_signature(0)
        avg_ms = st["total_ms"] / max(st["launches"], 1)
        return dict(ns=ns, solver=solver, xd=xd, bd=bd, step=step, n=n, dt=dt, steps=steps, st=st, fmt=fmt, avg_ms=avg_ms,
                    t_setup=t_setup, iters=int(solver.log.num_iters), dofs_per_s=n * steps / dt,
                    hist=np.array(solver.log.residuals[: solver.log.num_iters + 1]))

    def roof(r, bytes_key, label_extra=None, leg=None, kernel=None):
        ach = r["st"][bytes_key] / (r["avg_ms"] * 1e-3) / 1e9 if r["st"]["launches"] else None
        d = {"leg": leg, "leg_value": r["dofs_per_s"], "leg_ms_per_step": r["dt"] / r["steps"] * 1e3,
             "bound": "hbm", "kernel": kernel or kernel_label(r["fmt"]), "sweep_signature": r["fmt"].get("sweep_signature"),
             "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
             "frac": (ach / HBM_PEAK_GBS) if ach else None,
             "bytes_per_launch": r["st"][bytes_key], "avg_launch_ms": r["avg_ms"], "launches_timed": r["st"]["launches"],
             "event_stride": r["st"].get("prof_stride"),
             "rows": int(r["st"]["rows"]), "nnz": int(r["st"]["nnz"])}
        if label_extra:
            d["bytes_model"] = label_extra
        bv = r["st"].get("by_variant") or {}
        if len(bv) > 1 or (bv and "x_every_sweep" not in bv):
            # the sweeps of a pass alternate between two forms (x untouched / x updated with two increments); events sit on every
            # 7th launch (odd stride), so avg_launch_ms is the launch-weighted mean of both -- each form's own figure here
            # with each form's OWN bytes (gmg_get_kernel_stats_by_variant); the 12 B/nnz model has one figure for every form
            fb = (lambda v: v["layout_bytes"]) if bytes_key == "layout_bytes" else (lambda v: r["st"][bytes_key])
            d["by_variant"] = {k: dict(v, bytes_per_launch=fb(v), achieved=fb(v) / (v["avg_ms"] * 1e-3) / 1e9,
                                       frac=fb(v) / (v["avg_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS) for k, v in bv.items()}
        if r["st"].get("fused_passes"):
            d["note"] = ("this level is small enough to run every smoothing pass as ONE launch (sells_smooth_kernel): avg_launch_ms is "
                         "pass time / sweeps and the per-sweep byte models do not describe what moves")
        return d

    def q1_pair(cells, nlev, steps, warmup, want_generic, want_host_io, tag):
        """default + generic leg (+ host-vector leg) of one Q1 problem: the same blocks at every size and every N"""
        nc = (cells,) * 3
        t0 = time.perf_counter()
        H = po.build_hierarchy(nc, nlev, 1)
        n = H["mats"][0].shape[0]
        b = po.dirichlet_lift_rhs(nc, 1) if args.rhs == "lin" else po.random_rhs(n)
        t_asm = time.perf_counter() - t0
        D = leg(H, b, nlev, steps, warmup)
        ns = D["ns"]
        x = D["xd"].cpu().numpy()
        R = dict(H=H, b=b, D=D, x=x, n=n, nc=nc, t_asm=t_asm, l2=po.l2_error_sq(nc, 1, x) if args.rhs == "lin" and args.full else None)
        R["model_bytes"] = ns.P_ns.model_bytes()
        R["device_bytes"] = ns.P_ns.device_bytes()
        compressed = D["fmt"]["row_patterns"] or D["fmt"]["value_dictionary"] or D["fmt"]["idx16"]
        R["compressed"] = compressed
        rc = roof(D, "layout_bytes", "bytes the chosen layout moves per launch: matrix stream as stored + row-wise vectors, each once "
                                     "(gmg_kernel_stats.layout_bytes); NOT the 12 B/nnz model -- that stream does not exist in this layout", leg=tag + "default")
        rc["pairs_with"] = "value / ms_per_step"
        tr, src = committed_traffic(kernel_family(D["fmt"]), cells, nlev, int(D["st"]["rows"]), D["fmt"].get("sweep_signature"))
        rc["traffic"], rc["traffic_source"] = tr, src
        if tr:
            rc["traffic_GBs"] = tr / (D["avg_ms"] * 1e-3) / 1e9
            rc["traffic_frac"] = rc["traffic_GBs"] / HBM_PEAK_GBS
        rc["speedup_vs_12B_per_nnz_model"] = D["st"]["alg_bytes"] / D["st"]["layout_bytes"]
        R["roofline_compressed"] = rc
        if want_host_io:
            try:
                R["host_io"] = host_io_leg(torch, S, ns, b, D["dt"] / D["steps"] * 1e3, steps,
                                           f"the {tag or 'default '}leg's solves ({cells}^3 cells, {nlev} levels) with b / x as host arrays (GMG_MEM_HOST)")
            except Exception as e:
                R["host_io"] = {"error": str(e)[-300:]}
        R["per_level"] = []
        return R

    def generic_of(R, cells, nlev, steps, tag):
        G = leg(R["H"], R["b"], nlev, steps, 1, GENERIC_OPTIONS)
        xg = G["xd"].cpu().numpy()
        G["rel_diff_vs_default"] = float(np.linalg.norm(xg - R["x"]) / np.linalg.norm(R["x"]))
        G["ns"].P_ns.close()
        rl = roof(G, "alg_bytes", "SURVEY 8(d): B_sweep = 12 Z + 68 N (fp64 value + int32 column per stored nonzero; row-wise "
                                  "vectors each once), Z = stored nonzeros of the caller's operator", leg=tag + "generic")
        vbytes, cgbytes = R["model_bytes"]
        # SURVEY 8(d) model bytes of one whole solve of THIS leg / its time: must stay below the peak if the pair is self-consistent
        smb = cgbytes * G["iters"] + 12.0 * R["H"]["mats"][0].nnz + 52.0 * R["n"]
        rl["solve_model_bytes"] = smb
        rl["solve_model_GBps"] = smb / (G["dt"] / G["steps"]) / 1e9
        rl["pairs_with"] = "value_generic / ms_per_step_generic"
        tr, src = committed_traffic(kernel_family(G["fmt"]), cells, nlev, int(G["st"]["rows"]), G["fmt"].get("sweep_signature"))
        rl["traffic"], rl["traffic_source"] = tr, src
        if tr:
            rl["traffic_GBs"] = tr / (G["avg_ms"] * 1e-3) / 1e9
            rl["traffic_over_algorithmic"] = tr / G["st"]["alg_bytes"]
        return G, rl

    # =====================================================================================================
    if world > 1:
        from gridapsolvers_jl_amd import multigpu
        out = multigpu.run_bench(args, rank, world, local_rank)
        if not args.full:
            out["roofline"] = {"leg": "generic", "skipped": "runs with --full"}
        if rank == 0:
            if "cpu" in legs:
                # the per-GPU problem of this run (args.cells^3 cells, args.levels levels) on the host cores: a bounded number of solves
                try:
                    cb, _x, _nit, _h = cpu_baseline(args.cells, args.levels, "lin")
                    cb["sample"] = f"the per-GPU problem of this run ({args.cells}^3 cells, {args.levels} levels) on the host cores: " + cb["sample"]
                    out["cpu_baseline"] = cb
                except Exception as e:
                    out["cpu_baseline"] = {"error": str(e)[-300:]}
            if "weak_ref" in legs:
                # the same per-GPU problem on ONE GPU (rank 0, the others wait at the barrier below): the anchor of this line's weak scaling
                try:
                    Rw = q1_pair(args.cells, args.levels, max(3, args.steps // 2), 1, False, False, "weak_scaling_ref/")
                    W = Rw["D"]
                    out["weak_anchor_value"] = W["dofs_per_s"]
                    out["weak_anchor_ms_per_step"] = W["dt"] / W["steps"] * 1e3
                    out["weak_scaling_ref"] = {"workload": f"the per-GPU problem of this run on ONE GPU (rank 0 alone, after the distributed legs)",
                                               "value": W["dofs_per_s"], "ms_per_step": W["dt"] / W["steps"] * 1e3, "cg_iterations": W["iters"],
                                               "roofline_compressed": Rw["roofline_compressed"]}
                    W["ns"].P_ns.close()
                except Exception as e:
                    out["weak_anchor_value"] = None
                    out["weak_scaling_ref"] = {"error": str(e)[-300:]}
            else:
                out["weak_anchor_value"] = None
        dist.barrier()
        if rank == 0:
            emit(out, args.full)
        dist.destroy_process_group()
        return

    # ============================ N = 1 ====================================================================
    nlev = args.levels
    R = q1_pair(args.cells, nlev, args.steps, args.warmup, "generic" in legs, "host_io" in legs, "")
    D, H, b, n, x, ns = R["D"], R["H"], R["b"], R["n"], R["x"], R["D"]["ns"]
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, x, D["hist"])       # x and the history as the last timed solve left them
    vbytes, cgbytes = R["model_bytes"]
    copy_GBs = read_GBs = None
    if args.full:
        # the same sweep kernel on the coarser levels (report per level; these fit the Infinity Cache)
        per_level = []
        ns.P_ns.set_option("prof_stride", 7)     # (untimed runs: dense sampling)
        for lv in range(1, nlev - 1):
            ns.P_ns.profile(lv, True)
            for _ in range(2):
                D["step"]()
            torch.cuda.synchronize()
            stl = ns.P_ns.kernel_stats()
            ns.P_ns.profile(lv, False)
            if stl["launches"]:
                avg_l = stl["total_ms"] / stl["launches"]
                fused = int(stl.get("fused_passes", 0))
                rec = {"level": lv, "rows": int(stl["rows"]), "nnz": int(stl["nnz"]), "avg_sweep_ms": avg_l,
                       "one_launch_per_pass": bool(fused), "model_12B_nnz_GBs": stl["alg_bytes"] / (avg_l * 1e-3) / 1e9}
                if fused:
                    # sells_smooth_kernel: r, x, 1/diag stay in registers for the whole pass -- only s (8 B/row written, gathered
                    # back through L2/MALL) moves per sweep, so a bytes-per-sweep rate would be meaningless here
                    rec["avg_pass_ms"] = stl["total_ms"] / fused
                    rec["note"] = "whole smoothing pass in one launch; time per sweep = pass time / sweeps"
                else:
                    rec["layout_GBs"] = stl["layout_bytes"] / (avg_l * 1e-3) / 1e9
                per_level.append(rec)
        copy_GBs = ns.P_ns.stream_probe(1 << 30, 10)    # measured streaming ceiling of this box, same run, library's own copy kernel
        read_GBs = ns.P_ns.stream_probe_read(1 << 30, 10)   # ... and of a read-only stream (the sweeps read far more than they write)
        R["roofline_compressed"]["coarser_levels"] = per_level
        R["roofline_compressed"]["frac_of_copy_ceiling"] = (R["roofline_compressed"]["achieved"] / copy_GBs) if R["roofline_compressed"]["achieved"] else None

    out = {
        "metric": "DoFs/sec, CG+GMG V-cycle on 3D Poisson Q1",
        "value": D["dofs_per_s"],
        "unit": "DoFs/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": D["dt"] / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "headline_leg": "default",
        "legs": LEGS_NOTE,
        "rccl_ranks": 0,
        "devices": [dict(rank=0, local_rank=local_rank, device=torch.cuda.current_device(), name=torch.cuda.get_device_properties(torch.cuda.current_device()).name)],
        "weak_anchor_value": None,
        "config": {
            "workload": f"BASELINE configs[1]: 3D Poisson Q1 {args.cells}^3 cells, {nlev}-level GMG V-cycle, "
                        f"Richardson(Jacobi,10,2/3) pre=post, dense-inverse coarse solve, CG rtol={rtol:g}, "
                        f"rhs={'u=x1+x2 Dirichlet lift' if args.rhs == 'lin' else 'U(-1,1) seed 20240601'}",
            "value_is": "default leg: storage layout chosen by gmg_setup (" + D["fmt"]["layout"] + "); value_generic: same problem, "
                        "every structure-exploiting layout switched off (options pattern=0 vdict=0 idx16=0 opattern=0): the plain 12 B/nnz "
                        "(col,val) stream, what an operator without any repeating structure (unstructured mesh) gets",
            "dofs": n, "nnz": H["mats"][0].nnz, "levels": nlev, "cg_iterations": D["iters"],
            "dofs_x_iters_per_s": n * D["iters"] * args.steps / D["dt"],
            "l2_error_sq": R["l2"],
            "model_bytes_per_cg_iter": cgbytes, "model_bytes_per_vcycle": vbytes,
            "setup_s": D["t_setup"], "assembly_s": R["t_asm"], "device_bytes": R["device_bytes"],
            "operator_storage": D["fmt"],
            "measured_copy_ceiling_GBs": copy_GBs, "measured_read_ceiling_GBs": read_GBs,
        },
        "roofline_compressed": R["roofline_compressed"],
    }
    if "host_io" in R:
        out["host_io"] = R["host_io"]
        out["value_host_io"] = R["host_io"].get("value")
        out["ms_per_step_host_io"] = R["host_io"].get("ms_per_step")

    # ---------------- generic leg: same problem, plain 12 B/nnz stream (the layout SURVEY 8(d)'s byte model describes) ----
    G = None
    if "generic" in legs and R["compressed"]:
        G, roofline = generic_of(R, args.cells, nlev, max(3, args.steps // 2), "")
    elif "generic" in legs:
        G = D                                                # the setup chose the plain stream by itself
        roofline = roof(D, "alg_bytes", "SURVEY 8(d): B_sweep = 12 Z + 68 N", leg="default (no structure found: the generic layout)")
        roofline["pairs_with"] = "value / ms_per_step"
    else:
        roofline = {"leg": "generic", "skipped": "--no-generic / --legs" if args.full else "runs with --full"}
    if G is not None:
        roofline["measured_copy_ceiling_GBs"] = copy_GBs
        roofline["frac_of_copy_ceiling"] = roofline["achieved"] / copy_GBs if roofline.get("achieved") else None
        roofline["measured_read_ceiling_GBs"] = read_GBs
        roofline["frac_of_read_ceiling"] = roofline["achieved"] / read_GBs if roofline.get("achieved") else None
        out["value_generic"] = G["dofs_per_s"]
        out["ms_per_step_generic"] = G["dt"] / G["steps"] * 1e3
        out["config"].update(cg_iterations_generic=G["iters"], setup_s_generic=G["t_setup"], operator_storage_generic=G["fmt"],
                             generic_rel_diff_vs_default_solution=G.get("rel_diff_vs_default"),
                             solve_model_GBps_generic=roofline.get("solve_model_GBps"))
    out["roofline"] = roofline

    # ---------------- variable coefficient (every row distinct -> generic layout by itself) ------------------
    V = None
    if "varcoef" in legs:
        nc = R["nc"]
        t0 = time.perf_counter()
        Hv = po.build_hierarchy(nc, nlev, 1, kappa=po.smooth_kappa)
        uex = po.nodal_values(nc, 1)
        bv = Hv["mats"][0].matvec(uex)
        t_asm_v = time.perf_counter() - t0
        V = leg(Hv, bv, nlev, max(3, args.steps // 2), 1)
        xv = V["xd"].cpu().numpy()
        if V["fmt"]["layout"] == "SELL-O":
            rv = roof(V, "layout_bytes", "bytes the SELL-O layout moves per launch: 8 B/nnz values + 2 B/row pattern id + row-wise vectors "
                                         "(gmg_kernel_stats.layout_bytes); the 12 B/nnz model's column stream does not exist here", leg="variable_coefficient")
            rv["speedup_vs_12B_per_nnz_model"] = V["st"]["alg_bytes"] / V["st"]["layout_bytes"]
        else:
            rv = roof(V, "alg_bytes", "B_sweep = 12 Z + 68 N", leg="variable_coefficient")
        rv["layout_bytes_per_launch"] = V["st"]["layout_bytes"]
        rv["alg_bytes_per_launch_12B_model"] = V["st"]["alg_bytes"]
        trv, srcv = committed_traffic(kernel_family(V["fmt"]), args.cells, nlev, int(V["st"]["rows"]), V["fmt"].get("sweep_signature"))
        rv["traffic"], rv["traffic_source"] = trv, srcv
        out["variable_coefficient"] = {
            "workload": f"int kappa(x) grad u . grad v, kappa smooth in [0.5,1.75] at cell centres, Q1 {args.cells}^3, {nlev} levels "
                        f"re-discretised per level, rhs = A u_h(x1+x2), CG rtol={rtol:g}",
            "value": V["dofs_per_s"], "unit": "DoFs/s", "ms_per_step": V["dt"] / V["steps"] * 1e3, "steps": V["steps"],
            "cg_iterations": V["iters"], "operator_storage": V["fmt"], "setup_s": V["t_setup"], "assembly_s": t_asm_v,
            "max_abs_error_vs_exact": float(np.max(np.abs(xv - uex))), "roofline": rv,
        }
        V["ns"].P_ns.close()
        del Hv, bv

    ns.P_ns.close()
    del R["H"], H

    # ---------------- the per-GPU problem of the N > 1 runs (BASELINE configs[3]) on this one GPU ------------
    # `bench.py --gpus N` (N > 1) gives every GPU WS_CELLS^3 cells and WS_LEVELS levels; the weak-scaling efficiency of those lines
    # is to be read against THIS figure (same operator family, same smoother, same tolerances), not against configs[1] above.
    if "weak_ref" in legs and (args.cells, nlev) != (WS_CELLS, WS_LEVELS):
        try:
            Rw = q1_pair(WS_CELLS, WS_LEVELS, max(3, args.steps // 2), 1, "generic" in legs, "host_io" in legs, "weak_scaling_ref/")
            W = Rw["D"]
            wref = {"workload": f"3D Poisson Q1 {WS_CELLS}^3 cells on ONE GPU, {WS_LEVELS}-level GMG V-cycle, same smoother / tolerances: the per-GPU "
                                f"problem of `bench.py --gpus N`, N > 1 (BASELINE configs[3]: {2 * WS_CELLS}^3 cells on 2x2x2 GPUs)",
                    "value": W["dofs_per_s"], "unit": "DoFs/s", "ms_per_step": W["dt"] / W["steps"] * 1e3, "steps": W["steps"],
                    "dofs": W["n"], "cg_iterations": W["iters"], "l2_error_sq": Rw["l2"],
                    "operator_storage": W["fmt"], "setup_s": W["t_setup"], "assembly_s": Rw["t_asm"],
                    "device_bytes": Rw["device_bytes"], "roofline_compressed": Rw["roofline_compressed"]}
            if "host_io" in Rw:
                wref["host_io"] = Rw["host_io"]
                wref["value_host_io"] = Rw["host_io"].get("value")
            W["ns"].P_ns.close()
            if "generic" in legs:
                Gw, rgw = generic_of(Rw, WS_CELLS, WS_LEVELS, 3, "weak_scaling_ref/")
                wref.update(value_generic=Gw["dofs_per_s"], ms_per_step_generic=Gw["dt"] / Gw["steps"] * 1e3,
                            cg_iterations_generic=Gw["iters"], roofline=rgw)
                del Gw
            out["weak_scaling_ref"] = wref
            out["weak_anchor_value"] = wref["value"]
            out["weak_anchor_ms_per_step"] = wref["ms_per_step"]
            del Rw, W
        except Exception as e:          # a box without the memory for it still reports the headline
            out["weak_scaling_ref"] = {"error": str(e)[-300:]}
    elif (args.cells, nlev) == (WS_CELLS, WS_LEVELS):
        out["weak_anchor_value"] = out["value"]
        out["weak_anchor_ms_per_step"] = out["ms_per_step"]

    # ---------------- BASELINE configs[2]: Q2, patch smoother, FGMRES(5) ---------------------------------------
    if "config3" in legs:
        try:
            out["config3"] = config3_leg(torch, pkg, args)
        except Exception as e:
            out["config3"] = {"error": str(e)[-400:]}

    # ---------------- BASELINE configs[4] on one GPU: Stokes Q2/P1disc, block-triangular FGMRES + GMG -----------
    if "config5" in legs:
        try:
            out["config5"] = config5_leg(torch, pkg, args, "cpu" in legs)
        except Exception as e:
            out["config5"] = {"error": str(e)[-400:]}

    # ---------------- the product's exchange path over RCCL on this one GPU (a folded 8-rank partition, self messages) ----------
    if "rccl_loopback" in legs:
        try:
            out["rccl_loopback"] = rccl_loopback_leg(torch, pkg, args)
        except Exception as e:
            out["rccl_loopback"] = {"error": str(e)[-400:]}

    if "cpu" in legs:
        cb, xo, nit_o, hist_o = cpu_baseline(args.cells, nlev, args.rhs)
        out["cpu_baseline"] = cb
        out["config"]["iterations_match_cpu"] = bool(nit_o == D["iters"] and (G is None or nit_o == G["iters"]))
        out["config"]["rel_diff_vs_cpu_solution"] = float(np.linalg.norm(x - xo) / np.linalg.norm(xo))
        if V is not None:
            try:
                rvc, xvo = run_oracle_child(args.cells, nlev, "manufactured", "smooth", "seq", 1, 0.0, 1, True)
                out["variable_coefficient"]["iterations_match_cpu"] = bool(rvc["iters"] == V["iters"])
                out["variable_coefficient"]["rel_diff_vs_cpu_solution"] = float(np.linalg.norm(xv - xvo) / np.linalg.norm(xvo))
                out["variable_coefficient"]["cpu_single_thread_seconds"] = rvc["seconds"]
            except Exception as e:
                out["variable_coefficient"]["cpu_check_error"] = str(e)[-300:]
        if isinstance(out.get("config3"), dict) and "error" not in out["config3"]:
            try:
                c3 = out["config3"]
                cb3, x3o, nit3, hist3 = cpu_baseline(c3["cpu_check"]["cells"], c3["cpu_check"]["levels"], "lin", config3=True, limit_seq=8.0)
                cb3["sample"] = (f"BASELINE configs[2] shape at {c3['cpu_check']['cells']}^3 cells, {c3['cpu_check']['levels']} levels (the size the sequential "
                                 f"oracle affords in ~10 s): " + cb3["sample"])
                c3["cpu_baseline"] = cb3
                c3["cpu_check"]["iterations_match_cpu"] = bool(nit3 == c3["cpu_check"]["gpu_iters"])
                c3["cpu_check"]["max_rel_dev_of_residual_history"] = float(np.max(np.abs(np.asarray(c3["cpu_check"]["gpu_hist"])[: nit3 + 1] - hist3) / hist3))
                c3["cpu_check"]["rel_diff_vs_cpu_solution"] = float(np.linalg.norm(c3["cpu_check"].pop("gpu_x") - x3o) / np.linalg.norm(x3o))
            except Exception as e:
                out["config3"]["cpu_baseline"] = {"error": str(e)[-300:]}
    if isinstance(out.get("config3"), dict) and isinstance(out["config3"].get("cpu_check"), dict):
        out["config3"]["cpu_check"].pop("gpu_x", None)
    emit(out, args.full)


def config3_leg(torch, pkg, args):
    """BASELINE configs[2]: 3-D Poisson Q2, 5-level GMG, Richardson(PatchSolver,10,0.2) pre = post on every level, FGMRES(5), rtol 1e-6
    (test/LinearSolvers/GMGTests.jl:18-47,119-123).  Operators of >= 1e6 rows are streamed (gmg_set_operator_rows): nobody holds their
    CSR.  The timed kernel is the operator mat-vec of the patch sweep (r -= A dx: 125 entries per row), its byte model 12 Z + 28 N."""
    po, S, abi = pkg.poisson, pkg.solvers, pkg.abi
    cells, nlev, order = args.config3_cells, args.config3_levels, 2

    def setup(cells, nlev, stream_min_rows):
        nc = (cells,) * 3
        t0 = time.perf_counter()
        H = po.build_hierarchy(nc, nlev, order, stream_min_rows=stream_min_rows)
        t_asm = time.perf_counter() - t0
        t0 = time.perf_counter()
        sm, npatch = [], []
        for l in range(nlev - 1):
            pp, pd = po.vertex_star_patches(H["ncells"][l], order)
            npatch.append(int(pp.size - 1))
            sm.append(S.RichardsonSmoother(S.PatchSolver(pp, pd), 10, 0.2))
        t_patch = time.perf_counter() - t0
        b = po.dirichlet_lift_rhs(nc, order)
        gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sm, post_smoothers=sm, maxiter=1)
        solver = S.FGMRESSolver(5, gmg, maxiter=20, atol=1e-14, rtol=1e-6)
        t0 = time.perf_counter()
        ns = S.numerical_setup(S.symbolic_setup(solver, H["mats"][0]), H["mats"][0])
        t_setup = time.perf_counter() - t0
        del sm, gmg.pre_smoothers[:], gmg.post_smoothers[:]
        return H, b, solver, ns, dict(assembly_small_levels_s=t_asm, patch_tables_s=t_patch, numerical_setup_incl_stream_generation_s=t_setup), npatch

    H, b, solver, ns, tsetup, npatch = setup(cells, nlev, 1000000)
    n = b.size
    bd = torch.from_numpy(b).cuda()
    xd = torch.zeros_like(bd)
    torch.cuda.synchronize()
    steps = max(2, args.steps // 3)

    def step():
        xd.zero_(); torch.cuda.synchronize(); S.solve_(xd, ns, bd)
    step()
    ns.P_ns.set_option("prof_stride", prof_stride_for(steps, 50 * max(1, int(solver.log.num_iters))))   # rare samples: each costs the stream ~11 us
    ns.P_ns.profile(0, True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    st = ns.P_ns.kernel_stats()
    ns.P_ns.profile(0, False)
    yd = torch.zeros_like(bd)
    ns.P_ns.op_apply(0, abi.OP_A, xd, yd)
    true_rel = float(torch.linalg.vector_norm(bd - yd) / torch.linalg.vector_norm(bd))
    x = xd.cpu().numpy()
    fmt = ns.P_ns.level_format(0)
    avg_ms = st["total_ms"] / max(st["launches"], 1)
    ach = st["alg_bytes"] / (avg_ms * 1e-3) / 1e9 if st["launches"] else None
    lay = st["layout_bytes"] / (avg_ms * 1e-3) / 1e9 if st["launches"] else None
    tr, src = committed_traffic("sells_kernel_wide", cells, nlev, int(st["rows"]), None, order=2)
    rl = {"leg": "config3", "leg_value": n / dt, "leg_ms_per_step": dt * 1e3, "bound": "hbm",
          "kernel": "sellw_zwalk_kernel<EPI_SUB> on levels of >= 1e6 rows (sells_kernel<EPI_SUB,...,K=5,VD,WL> below): r -= A dx of the patch sweep -- Q2 "
                    "stiffness matrix, 125 entries per row, coded row-pattern table decoded per workgroup into LDS, the 25 windows of a row walked up the grid planes",
          "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": (ach / HBM_PEAK_GBS) if ach else None,
          "bytes_model": "SURVEY 8(d): r -= A dx = 12 Z + 28 N -- a (col,val) stream this layout does not have: `frac` > 1 means faster than streaming "
                         "the CSR would allow; see layout_GBs / traffic for what actually moves",
          "bytes_per_launch": st["alg_bytes"], "layout_bytes_per_launch": st["layout_bytes"], "layout_GBs": lay,
          "layout_frac": (lay / HBM_PEAK_GBS) if lay else None,
          "avg_launch_ms": avg_ms, "launches_timed": st["launches"], "rows": int(st["rows"]), "nnz": int(st["nnz"]),
          "traffic": tr, "traffic_source": src}
    if tr:
        rl["traffic_GBs"] = tr / (avg_ms * 1e-3) / 1e9
        rl["traffic_frac"] = rl["traffic_GBs"] / HBM_PEAK_GBS
    out = dict(workload=f"BASELINE configs[2]: 3D Poisson Q2 {cells}^3 cells, {nlev}-level GMG, Richardson(PatchSolver,10,0.2) pre=post, "
                        f"FGMRES(5) rtol=1e-6, rhs = u=x1+x2 Dirichlet lift" + ("" if cells == 256 else " (BASELINE size: --config3-cells 256)"),
               value=n / dt, unit="DoFs/s", ms_per_step=dt * 1e3, steps=steps, dofs=int(n), dofs_per_level=[int(M.shape[0]) for M in H["mats"]],
               patches_per_level=npatch, streamed_levels=[l for l, M in enumerate(H["mats"]) if hasattr(M, "row_blocks")],
               fgmres_iterations=int(solver.log.num_iters), flag=int(solver.log.flag),
               hist_rel=(solver.log.residuals[:solver.log.num_iters + 1] / solver.log.residuals[0]).tolist(),
               true_residual_rel=true_rel, l2_error_sq=po.l2_error_sq((cells,) * 3, order, x),
               setup=tsetup, operator_storage=fmt, device_GB=ns.P_ns.device_bytes() / 1e9, roofline=rl)
    ns.P_ns.close()
    del H, bd, xd, yd
    # the same configuration at the size the CPU oracle affords: iteration count, history and solution against the oracle (run in main)
    cc, cl = 32, 4
    H2, b2, solver2, ns2, _t, _np = setup(cc, cl, 20000)
    x2 = np.zeros_like(b2)
    S.solve_(x2, ns2, b2)
    out["cpu_check"] = dict(cells=cc, levels=cl, gpu_iters=int(solver2.log.num_iters),
                            gpu_hist=[float(v) for v in solver2.log.residuals[: solver2.log.num_iters + 1]], gpu_x=x2)
    ns2.P_ns.close()
    return out


def rccl_loopback_leg(torch, pkg, args):
    """FUNCTIONAL record (no scaling claim: one GPU): the 2x2x2 partition of a 3-D Q1 Poisson problem folded onto this GPU
    (partition.fold_ranks) and solved with CG + GMG through the product's own exchange path over RCCL -- pack kernel / fused pack in the
    boundary fix-up -> ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd on the communication stream -> event -> boundary fix-up,
    ncclAllReduce for every dot / norm and for the replicated coarse levels' residual (gmg_comm_set_loopback: a communicator of ONE rank,
    every neighbour is this rank itself).  Overlapped with the own x own kernels and in-stream; checked bit for bit against the same
    folded partition through the host-staged loopback.  Its times next to the unpartitioned solve of the same problem show what the
    partitioned path costs on one GPU (split kernels + exchanges + all-reduces), kernels and transport together."""
    import importlib
    pa, mg, po, S = (importlib.import_module(pkg.__name__ + "." + m) for m in ("partition", "multigpu", "poisson", "solvers"))
    per, nlev, W = args.loopback_cells, args.loopback_levels, 8
    cells = (2 * per,) * 3
    grid = pa.rank_grid(W, 3)
    rep_from, depths, _plan = mg.plan_partition(per, nlev, W)
    depths = [0] + list(depths[1:])          # finest level own | ghost (as at BASELINE config 4's size): its exchanges overlap the own x own kernel
    t0 = time.perf_counter()
    F = pa.fold_ranks([pa.build_local_hierarchy(cells, nlev, grid, r, 1, None, rep_from, depths, "jacobi") for r in range(W)])
    t_fold = time.perf_counter() - t0
    steps = max(3, args.steps // 2)

    def run(transport, overlap):
        old = os.environ.get("GMG_OVERLAP")
        os.environ["GMG_OVERLAP"] = "1" if overlap else "0"
        try:
            g = mg.DistributedGMG(cells, nlev, 0, 2, device_id=torch.cuda.current_device(), transport=transport, local_hierarchy=F, cells_global=cells)
        finally:
            os.environ.pop("GMG_OVERLAP", None) if old is None else os.environ.__setitem__("GMG_OVERLAP", old)
        b = torch.from_numpy(g.rhs_lin()).cuda()
        x = torch.zeros(g.n_own, dtype=torch.float64, device="cuda")

        def step():
            x.zero_(); torch.cuda.synchronize()
            return g.cg_solve(b, x, maxiter=20, atol=1e-14, rtol=1e-6)
        step()
        ex0, ar0 = g.comm_stats()
        torch.cuda.synchronize()
        ts = []
        for _ in range(steps):
            t0 = time.perf_counter()
            lg = step()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        dt = float(np.median(ts))                 # (median of the per-solve times: a functional record, and memory the earlier legs freed is still being returned)
        ex1, ar1 = g.comm_stats()
        rec = dict(ms_per_step=dt * 1e3, iters=int(lg.num_iters), exchanges_per_solve=(ex1 - ex0) / steps, allreduces_per_solve=(ar1 - ar0) / steps,
                   info=g.comm_info(), x=x.cpu().numpy(), err=float(np.max(np.abs(x.cpu().numpy() - g.exact_own()))), n=int(g.n_own),
                   sweep_signature=g.sweep_signature(0))
        g.close()
        return rec
    host = run("host_loopback", False)
    ovl = run("rccl_loopback", True)
    ins = run("rccl_loopback", False)
    # the same global problem unpartitioned on this GPU
    H = po.build_hierarchy(cells, nlev, 1)
    sm = [S.RichardsonSmoother(S.JacobiLinearSolver(), 10, 2.0 / 3.0)] * (nlev - 1)
    gm = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sm, post_smoothers=sm, coarsest_solver=S.LUSolver(), maxiter=1,
                           mode="preconditioner", cycle_type="v_cycle")
    sol = S.CGSolver(gm, maxiter=20, atol=1e-14, rtol=1e-6)
    ns = S.numerical_setup(S.symbolic_setup(sol, H["mats"][0]), H["mats"][0])
    bd = torch.from_numpy(po.dirichlet_lift_rhs(cells, 1)).cuda()
    xd = torch.zeros_like(bd)
    S.solve_(xd, ns, bd)
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        xd.zero_(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        S.solve_(xd, ns, bd)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    t_one = float(np.median(ts))
    xs = xd.cpu().numpy()
    ns.P_ns.close()
    gid = F["levels"][0].own_gid
    return dict(workload=f"3D Poisson Q1 {cells[0]}^3 cells ({ovl['n']} dofs), {nlev}-level GMG V-cycle, Richardson(Jacobi,10,2/3), CG rtol=1e-6: the 2x2x2 partition "
                         f"({per}^3 cells per rank; planner: replicated from level {rep_from}, halo depths {depths}) folded onto ONE GPU, every neighbour = this rank",
                rccl_ranks=int(ovl["info"]["rccl_comm_count"]), virtual_ranks=W, transport=ovl["info"]["transport"], steps=steps,
                cg_iterations=ovl["iters"], exchanges_per_solve=ovl["exchanges_per_solve"], allreduces_per_solve=ovl["allreduces_per_solve"],
                ms_per_step_overlapped=ovl["ms_per_step"], ms_per_step_in_stream=ins["ms_per_step"], ms_per_step_host_staged=host["ms_per_step"],
                ms_per_step_unpartitioned=t_one * 1e3,
                bitwise_equal_host_transport=bool(np.array_equal(ovl["x"], host["x"]) and np.array_equal(ins["x"], host["x"])),
                same_counts_as_host_transport=bool(ovl["exchanges_per_solve"] == host["exchanges_per_solve"] and ovl["allreduces_per_solve"] == host["allreduces_per_solve"]),
                iterations_match_unpartitioned=bool(ovl["iters"] == int(sol.log.num_iters)),
                rel_diff_vs_unpartitioned_solution=float(np.linalg.norm(ovl["x"] - xs[gid]) / np.linalg.norm(xs)),
                max_abs_error_vs_exact=ovl["err"], sweep_signature=ovl["sweep_signature"], fold_s=t_fold)


def config5_leg(torch, pkg, args, want_cpu):
    """BASELINE configs[4] on ONE GPU (its 8-GPU form needs the node): the reference application test/Applications/StokesGMG.jl:79-166 --
    lid-driven cavity, Q2 velocity / discontinuous P1 pressure, grad-div augmented velocity form (alpha = 1e3), FGMRES(20; atol 1e-10,
    rtol 1e-12) with the upper block-triangular preconditioner [A_uu (GMG)  -B^T ; 0  -1/alpha M_p (CG-Jacobi, 20 its, rtol 1e-6)],
    velocity GMG = maxiter 4, vertex-star patch smoothers Richardson(PatchSolver,10,0.2), patch-corrected prolongation with the grad-div rhs
    form, LU coarsest -- on synthesised inputs (gridapsolvers.jl_amd/stokes.py).  A step = one whole solve!(x, ns, b) from x = 0, b and x
    resident in HBM.  Checked in the same run: ||K x - b|| < 1e-7 (StokesGMG.jl:165) through scipy on the host; on an affordable size the
    oracle's iteration count / history / solution and its time (cpu_baseline, one thread: the oracle's patch solves are sequential)."""
    import importlib
    S, po = pkg.solvers, pkg.poisson
    st = importlib.import_module(pkg.__name__ + ".stokes")
    alpha = 1.0e3

    def make(n, nlev, with_K=False):
        t0 = time.perf_counter()
        # (inputs by stencil replication, stokes.stokes_system_fast: bitwise the scipy assembly, seconds instead of minutes)
        fast = n >= 8 and not (n & (n - 1))
        sysd = st.stokes_system_fast(n, alpha, with_K=with_K) if fast else st.stokes_system(n, alpha)
        Hv = st.velocity_hierarchy_fast(n, nlev, alpha) if fast else st.velocity_hierarchy(n, nlev, alpha)
        t_asm = time.perf_counter() - t0
        sm = [S.RichardsonSmoother(S.PatchSolver(pp, pd), 10, 0.2) for pp, pd in Hv["star_patches"]]
        interp = [S.PatchProlongationOperator(Hv["prolongations"][l], *Hv["interior_patches"][l], pivoting=True, rhs=Hv["graddiv"][l])
                  for l in range(nlev - 1)]
        gmg = S.GMGLinearSolver(Hv["mats"], interp, Hv["restrictions"], pre_smoothers=sm, post_smoothers=sm,
                                coarsest_solver=S.LUSolver(), maxiter=4, mode="preconditioner")
        solver_p = S.CGSolver(S.JacobiLinearSolver(), maxiter=20, atol=1e-14, rtol=1e-6)
        blocks = [[S.LinearSystemBlock(), S.LinearSystemBlock()], [S.LinearSystemBlock(), S.MatrixBlock(sysd["Mp_scaled"])]]
        Pd = S.BlockTriangularSolver(blocks, [gmg, solver_p], coeffs=[[1.0, 1.0], [0.0, 1.0]], half="upper")
        solver = S.FGMRESSolver(20, Pd, atol=1e-10, rtol=1e-12, maxiter=100)
        t0 = time.perf_counter()
        ns = S.numerical_setup(S.symbolic_setup(solver, sysd["A"]), sysd["A"])
        return sysd, Hv, solver, gmg, solver_p, ns, t_asm, time.perf_counter() - t0

    n, nlev = args.config5_cells, args.config5_levels
    sysd, Hv, solver, gmg, solver_p, ns, t_asm, t_setup = make(n, nlev)
    b = sysd["b"]
    N = b.size
    bd = torch.from_numpy(b).cuda()
    xd = torch.zeros_like(bd)
    torch.cuda.synchronize()
    steps = max(2, args.steps // 3)
    gv = ns.P_ns.block_ns[0]                         # the velocity block's GMG setup

    def step():
        xd.zero_(); torch.cuda.synchronize(); S.solve_(xd, ns, bd)
    step()
    gv.set_option("prof_stride", prof_stride_for(steps, 80 * max(1, int(solver.log.num_iters))))
    gv.profile(0, True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    kst = gv.kernel_stats()
    gv.profile(0, False)
    x = xd.cpu().numpy()
    nu, npp = sysd["sizes"]
    # norm(K x - b) block by block on the host (scipy): K = [A_uu A_up ; A_pu 0]
    Ab = sysd["A"]
    ru = Ab[0][0].matvec(x[:nu]) + Ab[0][1].matvec(x[nu:]) - b[:nu]
    rp = Ab[1][0].matvec(x[:nu]) - b[nu:]
    res = float(np.sqrt(ru @ ru + rp @ rp))
    fmt = gv.level_format(0)
    avg_ms = kst["total_ms"] / max(kst["launches"], 1)
    rl = None
    if kst["launches"]:
        ach = kst["alg_bytes"] / (avg_ms * 1e-3) / 1e9
        lay = kst["layout_bytes"] / (avg_ms * 1e-3) / 1e9
        # priced with the bytes the stored layout moves (the row-pattern form has no 12 B/nnz stream: that model would give frac > 1) next to
        # the PMC-measured HBM traffic of the same kernel at this size (profiles/traffic_latest.json, run_profile.sh --order 3)
        tr, src = committed_traffic("sells_kernel_wide", n, nlev, int(kst["rows"]), None, order=3)
        vec_MB = 8.0 * kst["rows"] / 1e6
        rl = {"leg": "config5", "bound": "hbm", "kernel": "r -= A dx of the velocity block's finest patch sweep (vector Q2 + grad-div: up to 50 entries per row), "
                                                           "sells_kernel<EPI_SUB, K=5, coded patterns decoded per workgroup into LDS>",
              "achieved": lay, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": lay / HBM_PEAK_GBS,
              "bytes_model": "bytes the stored layout moves per launch (pattern id + dx in + r in / out per row: gmg_kernel_stats.layout_bytes)",
              "bytes_per_launch": kst["layout_bytes"], "model_12B_per_nnz_bytes": kst["alg_bytes"], "model_12B_per_nnz_GBs": ach,
              "avg_launch_ms": avg_ms, "launches_timed": kst["launches"], "rows": int(kst["rows"]), "nnz": int(kst["nnz"]),
              "traffic": tr, "traffic_source": src,
              "note": f"one vector of this level is {vec_MB:.0f} MB: " + ("the sweep's operands (r, dx, x, patch tables) outgrow the 256 MB Infinity Cache" if vec_MB >= 60
                                                                            else "the level sits in the 256 MB Infinity Cache / L2s, the HBM roofline is an upper bound only")}
        if tr:
            rl["traffic_GBs"] = tr / (avg_ms * 1e-3) / 1e9
            rl["traffic_frac"] = rl["traffic_GBs"] / HBM_PEAK_GBS
    out = dict(workload=f"BASELINE configs[4] on one GPU: 2-D Stokes lid-driven cavity, Q2 / P1disc on {n}x{n} cells, alpha = {alpha:g}; FGMRES(20, atol 1e-10, "
                        f"rtol 1e-12) + upper block-triangular preconditioner; velocity: {nlev}-level GMG(maxiter 4, Richardson(PatchSolver,10,0.2) pre = post, "
                        f"patch-corrected prolongation (grad-div rhs), LU coarsest); pressure: CG-Jacobi(20, rtol 1e-6) on -1/alpha M_p",
               value=N / dt, unit="DoFs/s", ms_per_step=dt * 1e3, steps=steps, dofs=int(N), velocity_dofs=int(nu), pressure_dofs=int(npp),
               velocity_dofs_per_level=[int(M.shape[0]) for M in Hv["mats"]],
               fgmres_iterations=int(solver.log.num_iters), flag=int(solver.log.flag), gmg_iterations_last_application=int(gmg.log.num_iters),
               pressure_cg_iterations_last_application=int(solver_p.log.num_iters),
               residual_norm_host_check=res, reference_criterion="norm(A x - b) < 1e-7 (StokesGMG.jl:165)", criterion_met=bool(res < 1e-7),
               hist_rel=(solver.log.residuals[: solver.log.num_iters + 1] / solver.log.residuals[0]).tolist(),
               lid_velocity_max=float(x[:nu].max()), setup_s=t_setup, assembly_s=t_asm, operator_storage=fmt, roofline=rl)
    ns.P_ns.close()
    del sysd, Hv, bd, xd
    if want_cpu:
        # the same configuration at the size the sequential oracle affords: iterations, history, solution and time against it
        orc = entry.import_oracle()
        cn, cl = args.config5_cpu_cells, args.config5_cpu_levels     # 256 / 5: ~10 s of single-thread oracle work
        sysd, Hv, solver, gmg, solver_p, ns, _a, _s = make(cn, cl, with_K=True)
        b = sysd["b"]
        x = np.zeros(b.size)
        S.solve_(x, ns, b)
        osm = [orc.Smoother(orc.PATCH, 10, 0.2, pp, pd) for pp, pd in Hv["star_patches"]]
        go = orc.GMG(Hv["mats"], Hv["prolongations"], Hv["restrictions"], pre_smoothers=osm, maxiter=4, rtol=1e-8,
                     prolongation_patches=[(orc.PATCH, *Hv["interior_patches"][l], Hv["graddiv"][l]) for l in range(cl - 1)])
        nu, npp = sysd["sizes"]
        Po = orc.BlockPreconditioner([nu, npp], [go, (orc.BD_CG_JACOBI, sysd["Mp_scaled"], 20, 1e-14, 1e-6)],
                                     {(0, 1): (sysd["A"][0][1], 1.0), (1, 0): (sysd["A"][1][0], 0.0)}, orc.UPPER)
        Kc = po.CSR(sysd["K"].shape, sysd["K"].indptr, sysd["K"].indices, sysd["K"].data)
        t0 = time.perf_counter()
        xo, nit, flag, hist = orc.fgmres_solve(Kc, b, Pr=Po, m=20, maxiter=100, atol=1e-10, rtol=1e-12)
        t_cpu = time.perf_counter() - t0
        out["cpu_baseline"] = dict(value=b.size / t_cpu, unit="DoFs/s", cores=1, kind="port", seconds=t_cpu, iters=int(nit),
                                   sample=f"one full solve of the same configuration at {cn}x{cn} cells, {cl} levels ({b.size} dofs) by oracle/gmg_oracle.c, "
                                          f"single thread ({t_cpu:.2f} s)")
        out["cpu_check"] = dict(cells=cn, levels=cl, gpu_iters=int(solver.log.num_iters), iterations_match_cpu=bool(solver.log.num_iters == nit),
                                max_dev_of_residual_history_rel_r0=float(np.max(np.abs(solver.log.residuals[: nit + 1] - hist)) / hist[0]),
                                rel_diff_vs_cpu_solution=float(np.linalg.norm(x - xo) / np.linalg.norm(xo)))
        ns.P_ns.close()
    return out


if __name__ == "__main__":
    main()
