"""Builds tests/cpp/test_robust_wire.cpp against include/threshold_crypto.hpp + libtc_amd.so and runs it on the GPU: the robust
combiners on wire bytes (PublicKeySet::combine_signatures_robust_wire_batch / decrypt_robust_wire_batch) through the C++ host
mirror.  The fixture -- key set, compressed shares with planted faults, expected statuses / used / bad / results -- is made
here with the library's own entries and the rules of include/tc_amd.h (the model of tests/test_gpu_robust.py)."""
import os
import struct
import subprocess

import pytest

from test_gpu_robust import OK
from test_gpu_robust_wire import WireEnc, WireSig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_robust_wire.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_robust_wire")
LIBDIR = os.path.join(ROOT, "threshold_crypto_amd")


def _build():
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), SRC, "-o", EXE, "-L" + LIBDIR,
                    "-ltc_amd", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_robust_wire_compiles_and_links():
    """CPU-side: the C++ mirror of the wire-level robust combiners compiles against the C ABI and links the shared library."""
    _build()
    assert os.path.exists(EXE)


def _plant(plan):
    plan.absent(1, [0, 3])                 # holes: clean
    plan.wrong(2, 1, other=0)              # a wrong share inside S0, and one past it that the examination reports too
    plan.wrong(2, 6, other=0)
    plan.only(3, [2, 5])                   # too few present
    plan.off_curve(4, 0)                   # an x without a square root inside S0: examined, reported


def _marks(indices, N):
    return bytes(1 if i in indices else 0 for i in range(N))


@pytest.mark.gpu
def test_cpp_robust_wire_combiners(engine, tmp_path):
    _build()
    t, N, B = 2, 7, 5
    sw = WireSig(engine, t, N, B, 0xC99)
    ew = WireEnc(engine, t, N, B, 0xC9A, poly=sw.w.poly)                   # one key set for both halves
    fx = struct.pack("<III", t, N, B) + sw.w.commit.tobytes()
    plan = sw.plan()
    _plant(plan)
    want = plan.expect()
    assert [w[3] for w in want] == [False, False, True, False, True]       # clean jobs and fallback jobs
    for j in range(B):
        fx += struct.pack("<I", len(sw.w.msgs[j])) + sw.w.msgs[j]
        for i in range(N):
            fx += bytes([int(plan.present[j, i])]) + plan.shares[j, i].tobytes()
        fx += bytes([want[j][0]]) + _marks(want[j][1], N) + _marks(want[j][2], N)
        fx += sw.want[j].tobytes() if want[j][0] == OK else bytes([0xC0]) + bytes(95)
    fx += struct.pack("<I", sum(1 for w in want if w[3]))
    plan = ew.plan()
    _plant(plan)
    want = plan.expect()
    w = ew.w
    for j in range(B):
        lo, hi = int(w.off[j]), int(w.off[j + 1])
        fx += w.u[j].tobytes() + struct.pack("<I", hi - lo) + w.v[lo:hi].tobytes() + w.w[j].tobytes()
        for i in range(N):
            fx += bytes([int(plan.present[j, i])]) + plan.shares[j, i].tobytes()
        fx += bytes([want[j][0]]) + _marks(want[j][1], N) + _marks(want[j][2], N)
        fx += struct.pack("<I", len(w.plain[j])) + w.plain[j]
    fx += struct.pack("<I", sum(1 for x in want if x[3]))
    path = tmp_path / "robust_wire.bin"
    path.write_bytes(fx)
    r = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CPP-ROBUST-WIRE-OK" in r.stdout, r.stdout + r.stderr
