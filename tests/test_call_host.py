"""The call frame of the C ABI on the CPU: threshold_crypto_amd/csrc/tc_api.hip compiled unchanged by g++ against a stand-in
HIP header (tests/call/fake_hip), linked with a runtime that DEFERS every copy, memset and launch until somebody synchronises
(tests/call/fake_runtime.cpp) and with stub launchers (tests/call/call_host.cpp, a test harness -- not a product path), built
with the address and undefined-behaviour sanitizers and run as a program of its own.

The program drives every entry whose host decides in mid-call -- the combined and RLC verifiers, the records front ends, the
robust combiners share by share and by bisection, tc_dkg_verify_values_rlc_batch -- clean and with the last job failing, in
host and in device I/O, and fails the k-th host allocation of each call for k = 0, 1, 2, ... until the call gets through.  Every
injected run must answer TC_ERR_HOST with a message, leave no 8-byte window of a secret (seed, blame key, DKG values) in any
live device block, and leave a context that answers the next call like a fresh one; a copy that runs after its host side was
freed is a sanitizer report.  (The commit before the frame owned its host buffers fails here at once: heap-use-after-free in
the D2H copy that on_exception's synchronise lets run, and seed bytes left on the device after TC_ERR_HOST.)"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "threshold_crypto_amd", "csrc")
HERE = os.path.join(ROOT, "tests", "call")
UNIT = os.environ.get("TC_CALL_HOST_UNIT") or os.path.join(CSRC, "tc_api.hip")  # (another copy of the unit: what an earlier commit does here)
SOURCES = [os.path.join(HERE, n) for n in ("call_host.cpp", "fake_runtime.cpp")]
EXE = os.path.join(HERE, "call_host_main")


def _stale():
    deps = SOURCES + [UNIT, os.path.join(HERE, "fake_runtime.h"), os.path.join(HERE, "fake_hip", "hip", "hip_runtime.h"),
                      os.path.join(ROOT, "include", "tc_amd.h")]
    deps += [os.path.join(CSRC, n) for n in os.listdir(CSRC) if n.endswith(".h")]
    return not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps)


@pytest.fixture(scope="module")
def exe():
    if _stale():
        # the launchers the driven entries never reach stay unresolved: a stray call would crash loudly
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(HERE, "fake_hip"), "-x", "c++", UNIT] + SOURCES +
                       ["-Wl,--unresolved-symbols=ignore-all", "-o", EXE], check=True)
    return EXE


def test_every_failed_allocation_ends_the_call_cleanly(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "call_host: ok" in out.stdout, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    swept = re.findall(r"^  (\S+) +io (\d) fail (\d): (\d+) allocations swept", out.stdout, re.M)
    # 18 entries x {host, device I/O} x {clean, last job failing}, and the four records entries with a bad key-table entry
    assert len(swept) == 18 * 4 + 4, len(swept)
    # every sweep met at least one allocation to fail and ended far below the cap of 10 000 steps
    assert all(0 < int(k) < 1000 for _, _, _, k in swept), swept


def test_the_frame_adds_no_allocation_per_job(exe):
    """Host allocations of one uninjected call.  The two entries without a host decision allocate what they did before the frame
    owned anything (4 and 3: counted on the parent commit with this harness).  No driven entry allocates per job of the BATCH:
    from its small shape to B = 50 (47 more jobs) a call may differ by a few vector growths, not by tens.  (Only the last job
    ever falls back here, so this says nothing about allocations per FAILED job; the counts of the parent commit beside these
    are in profiles/call_frame_ab.txt.)"""
    out = subprocess.run([exe, "--counts"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    print(out.stdout)
    plain = dict(re.findall(r"^allocs (\S+) \(no host decision\) +host (\d+)", out.stdout, re.M))
    assert plain == {"verify_g2": "4", "combine_g2": "3"}, plain
    rows = re.findall(r"^allocs (\S+) +fail (\d): small (\d+)  B=50 (\d+)", out.stdout, re.M)
    assert len(rows) == 18 * 2, len(rows)
    for name, fail, small, large in rows:
        assert abs(int(large) - int(small)) < 10, (name, fail, small, large)
