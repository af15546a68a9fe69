"""tc_g1_sum_batch (Commitment::add_assign folded over the accepted parts, src/poly.rs:462-471, 895-898) at its two ends, in one
process on device-resident operands, input checks off (the operands are the library's own outputs):
  (a) 68 outputs x 200 terms   the public side of a DKG round at N = 200, degree 67: few outputs, long sums
  (b) 65 536 outputs x 4 terms many outputs, short sums: the batch alone fills the GPU
Legs: k_g1_sum with TC_SUM_PARTS lanes per output forced -- (a) 1, 4, 16, 64; (b) 1, 2 --, the library's default rule, and the only
form the library offered before: tc_g1_lincomb_batch with unit scalars on the same points.  A context reads TC_SUM_PARTS once, when
it is created, so every forced value has its own context.  All outputs are compared byte for byte before any time is reported.
Every leg is warmed, then the legs ALTERNATE inside each of the timed rounds; per leg the median and the spread (min .. max) of
tc_last_kernel_ms.  Prints the lines and writes them to --out.
usage: python tools/g1_sum_probe.py [--reps 5] [--out profiles/g1_sum_probe.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from threshold_crypto_amd.engine import Engine

SHAPES = [("a", 68, 200, (1, 4, 16, 64)), ("b", 65536, 4, (1, 2))]


def context(parts):
    saved = os.environ.get("TC_SUM_PARTS")
    if parts is None:
        os.environ.pop("TC_SUM_PARTS", None)
    else:
        os.environ["TC_SUM_PARTS"] = str(parts)
    try:
        e = Engine(0)
    finally:
        if saved is None:
            os.environ.pop("TC_SUM_PARTS", None)
        else:
            os.environ["TC_SUM_PARTS"] = saved
    e.set_timing(True)
    e.set_input_checks(False)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20261)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g1_sum_probe.txt"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least five timed rounds")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(a.seed)
    ctx = {p: context(p) for p in (None, 1, 2, 4, 16, 64)}
    base = ctx[None]
    lines = ["g1_sum_probe: device I/O, input checks off, %d timed rounds after %d warm-up round(s) of every leg, legs alternating; "
             "ms = tc_last_kernel_ms, median (min .. max)" % (a.reps, a.warmup), "device: " + base.version()]
    for tag, B, n, forced in SHAPES:
        fr = rng.integers(0, 256, size=(n * B, 32), dtype=np.uint8)
        fr[:, 31] &= 0x3f                                                # below 2^254 < r: canonical
        pts, st = base.g1_commitment(torch.from_numpy(fr).to(dev))
        base.sync()
        assert not bool(st.any())
        pts = pts.reshape(n, B, 96)                                      # term-major: what the sum reads
        by_job = pts.permute(1, 0, 2).contiguous()                       # job-major: what the linear combination reads
        one = np.zeros((B, n, 32), dtype=np.uint8)
        one[:, :, 0] = 1
        one = torch.from_numpy(one).to(dev)
        torch.cuda.synchronize()

        def sum_leg(e):
            def run():
                out, st_ = e.g1_sum(pts)
                ms = e.last_kernel_ms()
                e.sync()
                return out, st_, ms
            return run

        def lincomb():
            out, st_ = base.lincomb_g1(one, by_job)
            ms = base.last_kernel_ms()
            base.sync()
            return out, st_, ms

        legs = [("parts=%d" % p, sum_leg(ctx[p])) for p in forced] + [("default", sum_leg(base)), ("lincomb, unit scalars", lincomb)]
        ref = None
        for name, leg in legs:                                           # equal bytes first
            out, st_, _ = leg()
            assert not bool(st_.any()), name
            ref = out if ref is None else ref
            assert bool((out == ref).all()), name
        ms = {name: [] for name, _ in legs}
        for rep in range(a.warmup + a.reps):
            for name, leg in legs:
                t = leg()[2]
                if rep >= a.warmup:
                    ms[name].append(t)
        lines.append("(%s) %d outputs x %d terms; all legs: equal bytes" % (tag, B, n))
        for name, _ in legs:
            v = ms[name]
            lines.append("    %-22s %9.3f (%9.3f .. %9.3f)" % (name, statistics.median(v), min(v), max(v)))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
