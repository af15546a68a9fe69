"""include/threshold_crypto.hpp decrypt_shares_batch from a stand-alone program (tests/cpp/test_decrypt_shares.cpp): the fixture is
made here -- ciphertexts by the engine, the expected shares with the oracle's integers -- and the program checks the mirror's
answers."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import tc_oracle as o
from threshold_crypto_amd.engine import pack_messages

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def test_cpp_mirror(engine, tmp_path):
    rnd = random.Random(0xD5C)
    src = os.path.join(ROOT, "tests", "cpp", "test_decrypt_shares.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_decrypt_shares")
    libdir = os.path.join(ROOT, "threshold_crypto_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + libdir, "-ltc_amd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    S, B = 5, 6
    sks = [rnd.randrange(1, o.R) for _ in range(S)]
    pk = u8(o.g1_uncompressed(o.E1.mul(o.G1_GEN, rnd.randrange(1, o.R))))
    msgs = [bytes(rnd.randrange(256) for _ in range(j * 5 % 13)) for j in range(B)]      # ciphertext 0: an empty plaintext
    flat, off = pack_messages(msgs)
    r = np.stack([u8(rnd.randrange(1, o.R).to_bytes(32, "little")) for _ in range(B)])
    u, v, w, st = engine.encrypt(pk, r, flat, off)
    assert not st.any()
    w = w.copy()
    w[4] = w[3]                                                                          # a tampered w: no shares
    ok = [0 if j == 4 else 1 for j in range(B)]
    fx = struct.pack("<II", S, B) + b"".join(k.to_bytes(32, "little") for k in sks)
    for j in range(B):
        vj = bytes(v[int(off[j]):int(off[j + 1])])
        fx += bytes(u[j]) + struct.pack("<I", len(vj)) + vj + bytes(w[j])
    fx += bytes(ok)
    for j in range(B):
        if ok[j]:
            U = o.g1_from_uncompressed(bytes(u[j]))
            fx += b"".join(o.g1_uncompressed(o.E1.mul(U, k)) for k in sks)
    path = tmp_path / "fixture.bin"
    path.write_bytes(fx)
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "CPP-DECRYPT-SHARES-OK" in res.stdout, res.stdout + res.stderr
