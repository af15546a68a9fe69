"""The values check of distributed key generation (`bi_commit.evaluate(m, s) == g1 * val`, src/poly.rs:846-848) at N = 200
nodes, degree 67: B = 200 parts (one row commitment each) x n = 200 values, three ways in one process on device-resident
operands:
  (a) composed   what the entries before tc_dkg_verify_values_batch offer: tc_public_key_share_batch once per part with the row as
                 its commitment, one tc_g1_commitment_batch over all values, the comparison on the host
  (b) exact      tc_dkg_verify_values_batch
  (c) rlc        tc_dkg_verify_values_rlc_batch (one random linear combination per part)
The operands are made on the device by the library itself from --seed (random row polynomials -> tc_g1_commitment_batch,
tc_fr_poly_evaluate_batch).  The three answers are compared -- on honest values and on a copy with wrong values -- before any
time is reported.  The legs ALTERNATE inside every repetition after the warm-up rounds; per leg the host clock around the calls
(ending in tc_sync) and, beside it, the sum of tc_last_kernel_ms.  Prints min / median / max and writes the same lines to --out.
usage: python tools/dkg_verify_probe.py [--nodes 200] [--degree 67] [--reps 7] [--out profiles/dkg_verify_probe.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from threshold_crypto_amd.engine import Engine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--degree", type=int, default=67)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20260)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dkg_verify_probe.txt"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least five timed repetitions")
    e = Engine(0)
    e.set_timing(True)
    dev = torch.device("cuda", 0)
    B = n = a.nodes
    d = a.degree
    rng = np.random.default_rng(a.seed)
    coeff = rng.integers(0, 256, size=(B, d + 1, 32), dtype=np.uint8)
    coeff[:, :, 31] &= 0x3f                                                  # below 2^254 < r: canonical
    xs_host = np.tile(np.arange(1, n + 1, dtype=np.uint64), (B, 1))
    xs_fr = np.zeros((n, 32), dtype=np.uint8)
    xs_fr[:, :8] = np.arange(1, n + 1, dtype="<u8").view(np.uint8).reshape(n, 8)
    t_coeff = torch.from_numpy(coeff).to(dev)
    rows, st = e.g1_commitment(t_coeff.reshape(B * (d + 1), 32))
    vals, st2 = e.fr_poly_evaluate(t_coeff, torch.from_numpy(xs_fr).to(dev))
    e.sync()
    assert not bool(st.any()) and not bool(st2.any())
    rows = rows.reshape(B, d + 1, 96)
    xs = torch.from_numpy(xs_host.view(np.int64)).to(dev)
    idx = torch.from_numpy((xs_host[0] - 1).view(np.int64)).to(dev)           # tc_public_key_share_batch evaluates at idx + 1
    lied = vals.clone()
    lied[7, 3, 0] ^= 1
    lied[7, 150, 1] ^= 1
    lied[B - 1, n - 1, 2] ^= 1
    torch.cuda.synchronize()
    seed = bytes(range(32))

    def composed(v):
        ms, evals = 0.0, []
        for j in range(B):
            out, st_ = e.public_key_shares(rows[j], idx)
            ms += e.last_kernel_ms()
            evals.append((out, st_))
        g, st_g = e.g1_commitment(v.reshape(B * n, 32))
        ms += e.last_kernel_ms()
        e.sync()
        ev = torch.stack([o for o, _ in evals]).cpu().numpy()
        good = np.stack([s.cpu().numpy() == 0 for _, s in evals]) & (st_g.cpu().numpy() == 0).reshape(B, n)
        ok = (ev == g.cpu().numpy().reshape(B, n, 96)).all(axis=2) & good
        return ok.astype(np.uint8), 0, ms

    def exact(v):
        ok = e.dkg_verify_values(rows, xs, v)
        ms = e.last_kernel_ms()
        e.sync()
        return ok.cpu().numpy(), 0, ms

    def rlc(v):
        ok, nfb = e.dkg_verify_values_rlc(rows, xs, v, seed)
        ms = e.last_kernel_ms()
        e.sync()
        return ok.cpu().numpy(), nfb, ms

    legs = [("a_composed", composed), ("b_exact", exact), ("c_rlc", rlc)]
    lines = ["dkg_verify_probe: %d parts x %d values, degree %d (row commitments of %d points), device I/O, %d timed repetitions after %d "
             "warm-up round(s), legs alternating; ms per leg: host clock around the calls (ending in tc_sync) | sum of tc_last_kernel_ms"
             % (B, n, d, d + 1, a.reps, a.warmup), "device: " + e.version()]
    for checks in (True, False):
        e.set_input_checks(checks)
        # the three answers agree, on honest values and on values with three wrong ones in two parts
        want = np.ones((B, n), dtype=np.uint8)
        for name, leg in legs:
            ok, nfb, _ = leg(vals)
            assert (ok == want).all() and nfb == 0, name
        want[7, 3] = want[7, 150] = want[B - 1, n - 1] = 0
        for name, leg in legs:
            ok, nfb, _ = leg(lied)
            assert (ok == want).all() and nfb == (2 if name == "c_rlc" else 0), (name, nfb)
        wall = {name: [] for name, _ in legs}
        kern = {name: [] for name, _ in legs}
        for rep in range(a.warmup + a.reps):
            for name, leg in legs:
                t0 = time.perf_counter()
                _, _, ms = leg(vals)
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    wall[name].append(dt)
                    kern[name].append(ms)
        tag = "input checks on" if checks else "input checks off"
        base = wall["a_composed"]
        for name, _ in legs:
            w, k = wall[name], kern[name]
            note = ""
            if name != "a_composed":
                note = "   median against (a): %.2fx; (a) spread min %.3f .. max %.3f" % (statistics.median(base) / statistics.median(w), min(base), max(base))
            lines.append("%-16s %-10s host min %9.3f median %9.3f max %9.3f | kernels min %9.3f median %9.3f max %9.3f%s"
                         % (tag, name, min(w), statistics.median(w), max(w), min(k), statistics.median(k), max(k), note))
    e.set_input_checks(True)
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
