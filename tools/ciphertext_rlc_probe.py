"""Ciphertext::verify for a batch: the per-ciphertext entry (tc_ciphertext_verify_batch) against the opt-in random linear
combination (tc_ciphertext_verify_rlc_batch) at group = 16, 64, 256 -- one process, device-resident operands, B ciphertexts of
ThresholdEncWorkload, input checks on and off.  The variants ALTERNATE inside every repetition (per-job, g16, g64, g256, per-job,
...), after a warm-up round of every variant; the time of a call is tc_last_kernel_ms (device events around the call's
kernels).  Prints min / median / max per variant and writes the same lines to --out.
usage: python tools/ciphertext_rlc_probe.py [--batch 65536] [--reps 7] [--out profiles/ciphertext_rlc_probe.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from threshold_crypto_amd.engine import Engine
from threshold_crypto_amd.workload import ThresholdEncWorkload

GROUPS = (16, 64, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ciphertext_rlc_probe.txt"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least five timed repetitions")
    e = Engine(0)
    e.set_timing(True)
    B = a.batch
    wl = ThresholdEncWorkload(e, 3, 10, B)
    dev = torch.device("cuda", 0)
    u, v, w = (torch.from_numpy(x).to(dev) for x in (wl.u, wl.v, wl.w))
    off = torch.from_numpy(wl.off.view(np.int64)).to(dev)
    seed = bytes(range(32))
    variants = [("per_job", lambda: (e.ciphertext_verify(u, v, off, w), 0))]
    for g in GROUPS:
        variants.append(("rlc_g%d" % g, lambda g=g: e.ciphertext_verify_rlc(u, v, off, w, group=g, seed=seed)))
    lines = ["ciphertext_rlc_probe: B = %d ciphertexts (t = 3, N = 10), device I/O, %d timed repetitions after %d warm-up rounds, "
             "variants alternating; ms per call (tc_last_kernel_ms)" % (B, a.reps, a.warmup), "device: " + e.version()]
    for checks in (True, False):
        e.set_input_checks(checks)
        times = {name: [] for name, _ in variants}
        for rep in range(a.warmup + a.reps):
            for name, call in variants:
                ok, nfb = call()
                ms = e.last_kernel_ms()
                if rep == 0:
                    assert bool(ok.all()) and nfb == 0, (name, nfb)      # all valid: every group passes on the fast path
                if rep >= a.warmup:
                    times[name].append(ms)
        tag = "input checks on" if checks else "input checks off"
        floor = min(times["per_job"])
        for name, _ in variants:
            t = times[name]
            med = statistics.median(t)
            note = ""
            if name != "per_job":
                note = "   median %s the per-job minimum (%.3f): %.2fx" % ("BELOW" if med < floor else "not below", floor, floor / med)
            lines.append("%-16s %-8s min %8.3f  median %8.3f  max %8.3f   %9.0f ciphertexts/s at the median%s"
                         % (tag, name, min(t), med, max(t), B / (med * 1e-3), note))
    e.set_input_checks(True)
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
