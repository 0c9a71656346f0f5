"""The small dense part of (F)GMRES on the host (csrc/krylov_small.hpp: givens_lapack, ArnoldiLSQ) against a Python transcription
of the same formulas.  No GPU: tests/host/arnoldi_small_main.cpp is compiled with the system C++ compiler under AddressSanitizer and
UBSan (-ffp-contract=off, the library's flag) and run as an ordinary child process.  Both sides are IEEE double + * / sqrt in the same
order, so the comparison is equality of every number (a NaN matches a NaN)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "arnoldi_small_main.cpp")
SAFMN2 = 2.0 ** -485
SAFMX2 = 1.0 / SAFMN2
INF = float("inf")


# ---------------------------------------------------------------- the transcription
def jl_max(a, b):
    return a + b if (a != a or b != b) else (a if a > b else b)


def givens(f, g):
    """LinearAlgebra.givensAlgorithm(f, g) -> (c, s, r)"""
    if g == 0.0:
        return 1.0, 0.0, f
    if f == 0.0:
        return 0.0, 1.0, g
    f1, g1 = f, g
    scale = jl_max(abs(f1), abs(g1))
    if scale >= SAFMX2:
        count = 0
        while True:
            count += 1; f1 *= SAFMN2; g1 *= SAFMN2; scale = jl_max(abs(f1), abs(g1))
            if scale < SAFMX2 or count >= 20:
                break
        r = math.sqrt(f1 * f1 + g1 * g1); c = f1 / r; s = g1 / r
        for _ in range(count):
            r *= SAFMX2
    elif scale <= SAFMN2:
        count = 0
        while True:
            count += 1; f1 *= SAFMX2; g1 *= SAFMX2; scale = jl_max(abs(f1), abs(g1))
            if scale > SAFMN2:
                break
        r = math.sqrt(f1 * f1 + g1 * g1); c = f1 / r; s = g1 / r
        for _ in range(count):
            r *= SAFMN2
    else:
        r = math.sqrt(f1 * f1 + g1 * g1); c = f1 / r; s = g1 / r
    if abs(f) > abs(g) and c < 0.0:
        c, s, r = -c, -s, -r
    return c, s, r


def arnoldi_lsq(beta, cols):
    """FGMRESSolvers.jl:147-188 / GMRESSolvers.jl:150-190 on the given Hessenberg columns (1-based H as a dict)"""
    m = len(cols)
    H, g, c, s, betas = {}, [0.0] * (m + 1), [0.0] * m, [0.0] * m, []
    g[0] = beta
    for j in range(1, m + 1):
        for i in range(1, j + 2):
            H[i, j] = cols[j - 1][i - 1]
        for i in range(1, j):
            gm = c[i - 1] * H[i, j] + s[i - 1] * H[i + 1, j]
            H[i + 1, j] = -s[i - 1] * H[i, j] + c[i - 1] * H[i + 1, j]
            H[i, j] = gm
        c[j - 1], s[j - 1], _r = givens(H[j, j], H[j + 1, j])
        H[j, j] = c[j - 1] * H[j, j] + s[j - 1] * H[j + 1, j]; H[j + 1, j] = 0.0
        g[j] = -s[j - 1] * g[j - 1]; g[j - 1] = c[j - 1] * g[j - 1]
        betas.append(abs(g[j]))
    out = {("beta", str(j + 1)): v for j, v in enumerate(betas)}
    out.update({("c", str(j + 1)): v for j, v in enumerate(c)})
    out.update({("s", str(j + 1)): v for j, v in enumerate(s)})
    out.update({("g", str(i)): v for i, v in enumerate(g)})
    out.update({("r", "%d,%d" % k): v for k, v in H.items()})
    y = list(g)
    for i in range(m, 0, -1):
        acc = 0.0
        for k in range(i + 1, m + 1):
            acc += H[i, k] * y[k - 1]
        y[i - 1] = (y[i - 1] - acc) / H[i, i]
    out.update({("y", str(i)): y[i] for i in range(m)})
    return out


# ---------------------------------------------------------------- the program
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler on PATH (c++, g++, clang++)"
    exe = str(tmp_path_factory.mktemp("arnoldi_small") / "arnoldi_small_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC]
    # the sanitizer runtimes linked into the program where the compiler knows the flags (gcc; clang does so by default): nothing
    # has to be loaded ahead of it, whatever else the environment puts into a process
    for static in (["-static-libasan", "-static-libubsan"], []):
        done = subprocess.run(cmd + static, capture_output=True, text=True)
        if done.returncode == 0:
            break
    assert done.returncode == 0, done.stderr
    return exe


def run(program, cap0, grow, beta, cols):
    text = "%d %d %d %s\n" % (cap0, grow, len(cols), float(beta).hex())
    text += "\n".join(" ".join(float(v).hex() for v in col) for col in cols) + "\n"
    done = subprocess.run([program], input=text, capture_output=True, text=True, timeout=10)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr)   # the sanitizers report on stderr
    out = {}
    for line in done.stdout.splitlines():
        name, idx, val = line.split()
        out[name, idx] = float.fromhex(val) if "nan" not in val else float("nan")
    return out


def same(a, b):
    return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def check(program, beta, cols, cap0=None, grow=1):
    got = run(program, cap0 if cap0 is not None else len(cols) + 1, grow, beta, cols)
    ref = arnoldi_lsq(beta, cols)
    assert sorted(got) == sorted(ref)
    bad = [(k, got[k].hex(), ref[k].hex()) for k in ref if not same(got[k], ref[k])]
    assert not bad, bad
    return got


def random_columns(m, seed):
    rng = np.random.default_rng(seed)
    return [[float(v) for v in rng.uniform(-1.0, 1.0, j + 1)] for j in range(1, m + 1)]


# ---------------------------------------------------------------- cases
@pytest.mark.parametrize("m", [1, 2, 7])
def test_random_columns(program, m):
    check(program, 0.75, random_columns(m, 100 + m))


@pytest.mark.parametrize("grow", [1, 3])
def test_reserve_keeps_the_old_entries(program, grow):
    """capacity 3 (two columns), seven columns: the store grows by `grow` columns at a time and gives what a store of full size gives"""
    cols = random_columns(7, 107)
    grown = check(program, 0.75, cols, cap0=3, grow=grow)
    whole = check(program, 0.75, cols)
    assert all(same(grown[k], whole[k]) for k in whole)


def test_zero_subdiagonal(program):
    """g == 0: c = 1, s = 0, the residual norm drops to 0 (the lucky breakdown)"""
    cols = random_columns(3, 7)
    cols[1][2] = 0.0
    got = check(program, 2.0, cols)
    assert got["c", "2"] == 1.0 and got["s", "2"] == 0.0 and got["beta", "2"] == 0.0


def test_zero_diagonal(program):
    """f == 0: c = 0, s = 1"""
    got = check(program, 2.0, [[0.0, 0.5], [0.25, -0.5, 0.125]])
    assert got["c", "1"] == 0.0 and got["s", "1"] == 1.0 and got["r", "1,1"] == 0.5


def test_sign_rule(program):
    """|f| > |g| and f < 0: c, s and r change sign together, c > 0"""
    got = check(program, 1.0, [[-3.0, 1.0]])
    assert got["c", "1"] > 0.0 and got["s", "1"] < 0.0 and got["r", "1,1"] < 0.0


@pytest.mark.parametrize("e", [500, -500])
def test_rescaling_branches(program, e):
    """entries of 2^500 (scale >= safmx2) and 2^-500 (scale <= safmn2)"""
    u = 2.0 ** e
    got = check(program, 1.0, [[u, 0.5 * u], [1.5 * u, -u, 0.25 * u]])
    assert all(math.isfinite(v) for v in got.values())
    assert abs(got["c", "1"] - 2.0 / math.sqrt(5.0)) < 1e-15 and abs(got["s", "1"] - 1.0 / math.sqrt(5.0)) < 1e-15


def test_infinite_subdiagonal_returns(program):
    """the reference's cap of 20 rescaling steps: close_column returns (run() gives the child 10 s), with NaN where Julia has NaN"""
    got = check(program, 1.0, [[1.0, INF], [0.5, 0.25, 0.125]])
    assert got["c", "1"] == 0.0 and got["s", "1"] != got["s", "1"]
