"""tc_decrypt_shares_g1_batch (the decryption shares of B ciphertexts by n selected holders each, out of a table of N key shares:
SecretKeyShare::decrypt_share_no_verify src/lib.rs:460-462 per holder) in its two forms against what a caller could do before, in
one process on device-resident operands, input checks off (the points are the library's own outputs):
  (a) the per-ciphertext comb, forced           (a context created with TC_COMB_G1_MIN="1,1": k_comb_tables_g1 + k_comb_decrypt)
  (b) one arena ladder per share, forced        (TC_COMB_G1_MIN beyond every shape: k_g1_mul_gather)
  (c) tc_g1_mul_batch with ALL N scalars        (every share of every ciphertext, of which n are used)
  (d) tc_g1_mul_batch with S = n scalars        (the case where every ciphertext has the SAME subset)
Shapes: n = 68 of N = 200 at B = 4 096, 65 536 and 131 072; n = 4 of N = 10 at B = 65 536; then legs (a) and (b) alone at the
shapes between (SCAN), to place the thresholds of tc_launch.h.  The bytes of (a), (b) and (c) gathered are compared before any
time is reported.  Every leg is warmed, then the legs ALTERNATE inside each of the timed rounds; per leg the
median and the spread (min .. max) of the HOST clock around the call and the tc_sync that ends it.  Prints the lines and writes
them to --out.
usage: python tools/decrypt_shares_probe.py [--reps 5] [--out profiles/decrypt_shares_probe.txt]"""
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

SHAPES = [(68, 200, 4096), (68, 200, 65536), (68, 200, 131072), (4, 10, 65536)]
# legs (a) and (b) alone at the shapes between: where the comb starts to pay (tc_launch.h kCombG1MinHolders, kCombG1MinBatch)
SCAN = [(68, 200, 1024), (68, 200, 16384), (8, 200, 65536), (16, 200, 65536), (32, 200, 65536), (16, 200, 131072)]


def context(comb_min):
    """a context made under TC_COMB_G1_MIN (None: the library's constants)"""
    saved = os.environ.get("TC_COMB_G1_MIN")
    try:
        if comb_min is None:
            os.environ.pop("TC_COMB_G1_MIN", None)
        else:
            os.environ["TC_COMB_G1_MIN"] = comb_min
        e = Engine(0)
    finally:
        if saved is None:
            os.environ.pop("TC_COMB_G1_MIN", None)
        else:
            os.environ["TC_COMB_G1_MIN"] = saved
    e.set_input_checks(False)
    return e


def timed(call, e):
    def run():
        e.sync()
        t0 = time.perf_counter()
        res = call()
        e.sync()
        return res, (time.perf_counter() - t0) * 1e3
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20263)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decrypt_shares_probe.txt"))
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps: at least three timed rounds")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(a.seed)
    comb, ladders = context("1,1"), context("%d,%d" % (2 ** 63, 2 ** 63))
    lines = ["decrypt_shares_probe: device I/O, input checks off, %d timed rounds after %d warm-up round(s) of every leg, legs alternating; "
             "ms = host clock around the call and its tc_sync, median (min .. max)" % (a.reps, a.warmup), "device: " + comb.version()]

    def random_fr(count):
        fr = rng.integers(0, 256, size=(count, 32), dtype=np.uint8)
        fr[:, 31] &= 0x3f                                                # below 2^254 < r: canonical
        return fr

    for n, N, B, scan in [s + (False,) for s in SHAPES] + [s + (True,) for s in SCAN]:
        table = torch.from_numpy(random_fr(N)).to(dev)
        u, st = ladders.g1_commitment(torch.from_numpy(random_fr(B)).to(dev))
        ladders.sync()
        assert not bool(st.any())
        u = u.reshape(B, 96).contiguous()
        idx_np = np.stack([np.sort(rng.choice(N, size=n, replace=False)) for _ in range(B)]).astype(np.int64)
        idx = torch.from_numpy(idx_np).to(dev)
        first_n = table[:n].contiguous()
        torch.cuda.synchronize()
        legs = [("(a) comb, forced", timed(lambda: comb.decrypt_shares_g1(table, idx, u), comb)),
                ("(b) gather ladders, forced", timed(lambda: ladders.decrypt_shares_g1(table, idx, u), ladders)),
                ("(c) g1_mul, all N = %d scalars" % N, timed(lambda: ladders.g1_mul(table, u), ladders)),
                ("(d) g1_mul, S = n = %d scalars" % n, timed(lambda: ladders.g1_mul(first_n, u), ladders))]
        if scan:
            legs = legs[:2]
        (out_a, st_a), _ = legs[0][1]()                                  # equal bytes first
        (out_b, st_b), _ = legs[1][1]()
        assert not bool(st_a.any()) and not bool(st_b.any())
        assert bool((out_a == out_b).all()), "comb != ladders"
        if not scan:
            (out_c, st_c), _ = legs[2][1]()
            rows = torch.arange(B, device=dev)[:, None]
            assert not bool(st_c.any()) and bool((out_c[rows, idx] == out_a).all()), "g1_mul gathered != comb"
            del out_c, st_c
        del out_a, out_b, st_a, st_b
        ms = {name: [] for name, _ in legs}
        for rep in range(a.warmup + a.reps):
            for name, leg in legs:
                res, t = leg()
                del res
                if rep >= a.warmup:
                    ms[name].append(t)
        lines.append("n = %d of N = %d holders, B = %d ciphertexts; %s: equal bytes" % (n, N, B, "(a) and (b)" if scan else "(a), (b) and (c) gathered"))
        for name, _ in legs:
            v = ms[name]
            lines.append("    %-34s %10.3f (%10.3f .. %10.3f)" % (name, statistics.median(v), min(v), max(v)))
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f_:
        f_.write(text)


if __name__ == "__main__":
    main()
