"""Builds tests/cpp/test_verify_dshare_records.cpp against include/threshold_crypto.hpp + libtc_amd.so and runs it on the GPU:
decryption-share verification under many key shares (PublicKeyShare::verify_decryption_share_records_batch) through the C++
host mirror.  The fixture -- ragged records, all valid at three group sizes and with one forged record first and last in a
group, and what each record must answer (the C oracle's verify_decryption_share, as in tests/test_gpu_verify_dshare_records.py)
-- is made here with the library's own entries; the empty inputs are the program's own."""
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_verify_dshare_records.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_verify_dshare_records")
LIBDIR = os.path.join(ROOT, "threshold_crypto_amd")


def _build():
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), SRC, "-o", EXE, "-L" + LIBDIR,
                    "-ltc_amd", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_verify_dshare_records_compiles_and_links():
    """CPU-side: the C++ mirror of the ragged decryption-share verification compiles against the C ABI and links the shared library."""
    _build()
    assert os.path.exists(EXE)


def _pack(case, group, bad):
    want = case.expect()
    assert sorted(np_flat(want)) == sorted(bad)
    fx = struct.pack("<II", case.M, group)
    for m in range(case.M):
        fx += case.u[m].tobytes() + struct.pack("<I", len(case.v[m])) + case.v[m] + case.w[m].tobytes() + struct.pack("<I", case.lens[m])
        for r in case.records_of(m):
            fx += case.pks[int(case.key_idx[r])].tobytes() + case.shares[r].tobytes() + bytes([int(want[r])])
    return fx + struct.pack("<I", len(case.group_records(group, bad)))


def np_flat(want):
    return [r for r in range(len(want)) if not want[r]]


@pytest.mark.gpu
def test_cpp_verify_dshare_records(engine, tmp_path):
    from test_gpu_verify_dshare_records import K, Case, RAGGED, World
    _build()
    world = World(engine)
    cases = [_pack(Case(world, RAGGED), group, []) for group in (3, 1, 64)]                    # all valid
    for where in ("first", "last"):                                                            # the group {3, 4, 5} of group = 3
        for kind in ("other_node", "other_ciphertext", "wrong_key"):
            case = Case(world, RAGGED)
            r = case.rec(3, 0) if where == "first" else case.rec(4, 6)
            m, k = case.ct_of[r], int(case.key_idx[r])
            if kind == "other_node":
                case.shares[r] = world.share[m, (k + 1) % K]
            elif kind == "other_ciphertext":
                case.shares[r] = world.share[m + 2, k]
            else:
                case.key_idx[r] = (k + 3) % K
            cases.append(_pack(case, 3, [r]))
    path = tmp_path / "verify_dshare_records.bin"
    path.write_bytes(struct.pack("<I", len(cases)) + b"".join(cases))
    r = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CPP-VERIFY-DSHARE-RECORDS-OK" in r.stdout, r.stdout + r.stderr
