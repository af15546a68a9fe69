"""Builds tests/cpp/test_verify_records.cpp against include/threshold_crypto.hpp + libtc_amd.so and runs it on the GPU: batch
verification under many keys (PublicKey::verify_records_batch) through the C++ host mirror.  The fixture -- ragged records with
one forged signature, and what each record must answer (the C oracle's verify, as in tests/test_gpu_verify_records.py) -- is
made here with the library's own entries."""
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_verify_records.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_verify_records")
LIBDIR = os.path.join(ROOT, "threshold_crypto_amd")


def _build():
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), SRC, "-o", EXE, "-L" + LIBDIR,
                    "-ltc_amd", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_verify_records_compiles_and_links():
    """CPU-side: the C++ mirror of the ragged batch verification compiles against the C ABI and links the shared library."""
    _build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_verify_records(engine, tmp_path):
    from test_gpu_verify_records import Case, RAGGED, World
    import c_oracle as c
    _build()
    world = World(engine)
    case = Case(world, RAGGED)
    forged = case.rec(4, 2)
    case.sigs[forged] = world.sig[5, int(case.key_idx[forged])]                # the key's signature of another message
    group = 3
    fx = struct.pack("<II", case.M, group)
    for m in range(case.M):
        fx += struct.pack("<I", len(world.msgs[m])) + world.msgs[m] + struct.pack("<I", case.lens[m])
        for r in range(case.rec(m), case.rec(m + 1)):
            pk = case.pks[int(case.key_idx[r])]
            want = c.verify(bytes(pk), bytes(case.sigs[r]), world.msgs[m])
            assert want == (0 if r == forged else 1)
            fx += pk.tobytes() + case.sigs[r].tobytes() + bytes([want])
    fx += struct.pack("<I", len(case.group_records(group, [forged])))
    path = tmp_path / "verify_records.bin"
    path.write_bytes(fx)
    r = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CPP-VERIFY-RECORDS-OK" in r.stdout, r.stdout + r.stderr
