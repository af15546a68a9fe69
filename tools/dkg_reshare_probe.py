"""tc_g1_weighted_sum_batch and tc_dkg_reshare_batch (the accepted parts of a resharing summed with Lagrange weights: `Poly * Fr`
src/poly.rs:210-254, Commitment::add_assign :462-471, the finalisation :870-876, 895-898) at the library's DKG shapes, in one process
on device-resident operands, input checks off (the operands are the library's own outputs):
  (a) 68 outputs x 68 terms    a resharing out of t_old = 67 into degree 67: exactly the t_old + 1 dealers that are combined
  (b) 68 outputs x 200 terms   the weighted sum over all 200 parts of the large DKG shape
Legs of the primitive: k_g1_wsum with TC_SUM_PARTS lanes per output forced (1, 4, 16, 64) and ONE slice (TC_WSUM_SLICES=1: one
group of lanes per output); the library's default rule, which at these shapes is 64 lanes and 2 / 4 slices per output; the
composition the library offered before -- tc_g1_lincomb_batch on the gathered points with the weights replicated per output (the
baseline); tc_g1_sum_batch on the same points (the floor: no multiplications).  Then the whole calls side by side:
tc_dkg_reshare_batch and tc_dkg_generate_batch over the same P parts of degree 67 (P = 68 and 200, t_old = 67, one sample set of
68 values per part), where the resharing combines the first 68 accepted parts.  A context reads TC_SUM_PARTS and TC_WSUM_SLICES once, when it
is created, so every forced value has its own context.  All outputs of the primitive's legs are compared byte for byte before any
time is reported, and the resharing's new commitment must keep coefficient 0 of the old one.  Every leg is warmed, then the legs
ALTERNATE inside each of the timed rounds; per leg the median and the spread (min .. max) of tc_last_kernel_ms.  Prints the lines
and writes them to --out.
usage: python tools/dkg_reshare_probe.py [--reps 5] [--out profiles/dkg_reshare_probe.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from threshold_crypto_amd.api import _R
from threshold_crypto_amd.engine import Engine

SHAPES = [("a", 68, 68), ("b", 68, 200)]
FORCED = (1, 4, 16, 64)
T_OLD = 67


def context(parts, slices):
    """a context made under TC_SUM_PARTS / TC_WSUM_SLICES (None: the library's rule)"""
    env = {"TC_SUM_PARTS": parts, "TC_WSUM_SLICES": slices}
    saved = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        e = Engine(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    e.set_timing(True)
    e.set_input_checks(False)
    return e


def fr_rows(vals):
    return np.stack([np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8) for v in vals])


def horner(coeff, x):
    r = 0
    for c in reversed(coeff):
        r = (r * x + c) % _R
    return r


def timed(call, e):
    def run():
        res = call()
        ms = e.last_kernel_ms()
        e.sync()
        return res, ms
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20262)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dkg_reshare_probe.txt"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least five timed rounds")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(a.seed)
    ctx = {p: context(p, 1) for p in FORCED}                             # one group of lanes per output: the lane rule alone
    base = context(None, None)                                           # the library's rule: lanes and slices
    lines = ["dkg_reshare_probe: device I/O, input checks off, %d timed rounds after %d warm-up round(s) of every leg, legs alternating; "
             "ms = tc_last_kernel_ms, median (min .. max)" % (a.reps, a.warmup), "device: " + base.version()]

    def report(legs):
        ms = {name: [] for name, _ in legs}
        for rep in range(a.warmup + a.reps):
            for name, leg in legs:
                t = leg()[1]
                if rep >= a.warmup:
                    ms[name].append(t)
        for name, _ in legs:
            v = ms[name]
            lines.append("    %-34s %9.3f (%9.3f .. %9.3f)" % (name, statistics.median(v), min(v), max(v)))

    def random_fr(count):
        fr = rng.integers(0, 256, size=(count, 32), dtype=np.uint8)
        fr[:, 31] &= 0x3f                                                # below 2^254 < r: canonical
        return fr

    for tag, B, n in SHAPES:
        # ---- the primitive ----
        pts, st = base.g1_commitment(torch.from_numpy(random_fr(n * B)).to(dev))
        base.sync()
        assert not bool(st.any())
        pts = pts.reshape(n, B, 96)                                      # term-major: what the sums read
        by_job = pts.permute(1, 0, 2).contiguous()                       # job-major: what the linear combination reads
        w = random_fr(n)
        w_dev = torch.from_numpy(w).to(dev)
        w_rep = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(w[None], (B, n, 32)))).to(dev)
        torch.cuda.synchronize()
        legs = [("weighted sum, parts=%d, 1 slice" % p, timed(lambda e=ctx[p]: e.g1_weighted_sum(pts, w_dev), ctx[p])) for p in FORCED]
        legs += [("weighted sum, default rule", timed(lambda: base.g1_weighted_sum(pts, w_dev), base)),
                 ("lincomb composition (baseline)", timed(lambda: base.lincomb_g1(w_rep, by_job), base))]
        ref = None
        for name, leg in legs:                                           # equal bytes first
            (out, st_), _ = leg()
            assert not bool(st_.any()), name
            ref = out if ref is None else ref
            assert bool((out == ref).all()), name
        legs.append(("plain sum, no weights (floor)", timed(lambda: base.g1_sum(pts), base)))
        lines.append("(%s) %d outputs x %d terms; the weighted legs and the composition: equal bytes" % (tag, B, n))
        report(legs)

        # ---- the whole calls: P = n parts of degree B - 1, old key set of degree T_OLD ----
        degree, P, n_v = B - 1, n, B
        nco = (degree + 1) * (degree + 2) // 2
        f = [int.from_bytes(bytes(r), "little") for r in random_fr(T_OLD + 1)]
        coeff = random_fr(P * nco).reshape(P, nco, 32)
        for p in range(P):                                               # dealer p is old node p: its constant term is f(p + 1)
            coeff[p, 0] = fr_rows([horner(f, p + 1)])[0]
        both, st = base.g1_commitment(torch.from_numpy(np.concatenate([fr_rows(f), coeff.reshape(P * nco, 32)])).to(dev))
        base.sync()
        assert not bool(st.any())
        old_commit, commits = both[:T_OLD + 1].contiguous(), both[T_OLD + 1:].reshape(P, nco, 96).contiguous()
        dealer_idx = torch.from_numpy(np.arange(P, dtype=np.int64)).to(dev)
        xs = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.arange(1, n_v + 1, dtype=np.int64)[None], (P, n_v)))).to(dev)
        vals = torch.from_numpy(random_fr(P * n_v).reshape(P, n_v, 32)).to(dev)  # any canonical values interpolate to SOME row
        torch.cuda.synchronize()
        reshare = timed(lambda: base.dkg_reshare(old_commit, dealer_idx, commits, degree, None, xs, vals), base)
        generate = timed(lambda: base.dkg_generate(commits, degree, None, xs, vals), base)
        (out, share, used, st_, status), _ = reshare()
        assert int(status.cpu()[0]) == 0 and not bool(st_.any()) and int(used.sum()) == T_OLD + 1
        assert bool((out[0] == old_commit[0]).all())                     # the master key does not move
        (out, share, st_), _ = generate()
        assert not bool(st_.any())
        lines.append("(%s) the whole call: %d parts of degree %d, t_old = %d, %d samples per part" % (tag, P, degree, T_OLD, n_v))
        report([("tc_dkg_reshare_batch", reshare), ("tc_dkg_generate_batch", generate)])
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f_:
        f_.write(text)


if __name__ == "__main__":
    main()
