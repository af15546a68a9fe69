"""Builds tests/cpp/test_robust_bisect.cpp against include/threshold_crypto.hpp + libtc_amd.so and runs it on the GPU: blame by
bisection (set_blame_bisect / blame_bisect / last_blame_stats) around the robust combiners of the C++ host mirror.  The fixture --
key set, shares with planted faults, expected statuses / used / bad / results, and the pairing checks and rounds of the search --
is made here with the library's own entries, the rules of include/tc_amd.h (the model of tests/test_gpu_robust.py) and the rule
of csrc/tc_blame.h (the model of tests/test_blame_host.py)."""
import os
import struct
import subprocess

import pytest

from test_gpu_robust import EncWorld, OK, SigWorld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_robust_bisect.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_robust_bisect")
LIBDIR = os.path.join(ROOT, "threshold_crypto_amd")


def _build():
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), SRC, "-o", EXE, "-L" + LIBDIR,
                    "-ltc_amd", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_robust_bisect_compiles_and_links():
    """CPU-side: the C++ mirror of the three context functions compiles against the C ABI and links the shared library."""
    _build()
    assert os.path.exists(EXE)


def _plant(plan):
    plan.absent(1, [0, 3])                 # holes
    plan.wrong(2, 1, other=0)              # a wrong share inside S0, and one past it that the examination reports too
    plan.wrong(2, 6, other=0)
    plan.only(3, [2, 5])                   # too few present
    plan.wrong(4, 6, other=0)              # past S0: clean, not reported
    plan.off_curve(0, 2)                   # does not decode: bad without a check, the root range of its job passes


def _marks(indices, N):
    return bytes(1 if i in indices else 0 for i in range(N))


@pytest.mark.gpu
def test_cpp_robust_bisect(engine, tmp_path):
    from test_gpu_robust_bisect import BPlan, expected_stats
    _build()
    t, N, B = 2, 7, 5
    sw = SigWorld(engine, t, N, B, 0xC99)
    ew = EncWorld(engine, t, N, B, 0xC9A, poly=sw.poly)                    # one key set for both halves
    fx = struct.pack("<III", t, N, B) + sw.commit.tobytes()
    plan = BPlan(B, N, t, sw.shares)
    _plant(plan)
    want = plan.expect()
    for j in range(B):
        fx += struct.pack("<I", len(sw.msgs[j])) + sw.msgs[j]
        for i in range(N):
            fx += bytes([int(plan.present[j, i])]) + plan.shares[j, i].tobytes()
        fx += bytes([want[j][0]]) + _marks(want[j][1], N) + _marks(want[j][2], N)
        fx += sw.want[j].tobytes() if want[j][0] == OK else bytes([0x40]) + bytes(191)
    checks, rounds, per_job = expected_stats(plan, want)
    assert per_job[0] == (1, 1) and checks > 1
    fx += struct.pack("<III", sum(1 for w in want if w[3]), checks, rounds)
    plan = BPlan(B, N, t, ew.shares)
    _plant(plan)
    want = plan.expect()
    for j in range(B):
        lo, hi = int(ew.off[j]), int(ew.off[j + 1])
        fx += ew.u[j].tobytes() + struct.pack("<I", hi - lo) + ew.v[lo:hi].tobytes() + ew.w[j].tobytes()
        for i in range(N):
            fx += bytes([int(plan.present[j, i])]) + plan.shares[j, i].tobytes()
        fx += bytes([want[j][0]]) + _marks(want[j][1], N) + _marks(want[j][2], N)
        fx += struct.pack("<I", len(ew.plain[j])) + ew.plain[j]
    checks, rounds, _ = expected_stats(plan, want)
    fx += struct.pack("<III", sum(1 for w in want if w[3]), checks, rounds)
    path = tmp_path / "robust_bisect.bin"
    path.write_bytes(fx)
    r = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CPP-ROBUST-BISECT-OK" in r.stdout, r.stdout + r.stderr
