"""include/threshold_crypto.hpp dkg_reshare from a stand-alone program (tests/cpp/test_dkg_reshare.cpp): the fixture is made here
with the oracle's integers, the program checks the mirror's answers and its exceptions."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import tc_oracle as o

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror(engine, tmp_path):
    from test_gpu_dkg_reshare import Scene, gen_mul
    rnd = random.Random(0xC99)
    src = os.path.join(ROOT, "tests", "cpp", "test_dkg_reshare.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_dkg_reshare")
    libdir = os.path.join(ROOT, "threshold_crypto_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + libdir, "-ltc_amd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    s = Scene(engine, rnd, 2, [4, 0, 6, 2, 1], 1, node=2)
    accept = [1, 0, 1, 1, 1]
    used, col, share = s.expect(accept)
    fx = struct.pack("<IIII", s.t_old, s.degree, s.P, s.xs.shape[1]) + s.old_commit.tobytes() + s.dealer_idx.tobytes() + bytes(accept)
    fx += s.commits.tobytes() + s.xs.tobytes() + s.vals.tobytes()
    fx += b"".join(gen_mul(c) for c in col) + share.to_bytes(32, "little") + bytes(used)
    path = tmp_path / "fixture.bin"
    path.write_bytes(fx)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CPP-RESHARE-OK" in r.stdout, r.stdout + r.stderr
