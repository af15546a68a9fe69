"""Pass 2 of the robust combiner share by share against blame by bisection (tc_ctx_set_blame_bisect): the SAME library, the same
context and identical inputs in both modes -- tc_combine_signatures_robust_batch, shares in HBM, input checks off, every share
present; a "bad job" holds another message's share in its first k slots (k = 1, 3: slot 0 lies inside S0, so the job is examined).
Shapes are those of tools/robust_combine_probe.py; one worst case (every share of every job bad) at t = 67, N = 200, 256 jobs.
Each timing is a host clock around a call that ends in tc_sync; one warm-up of every case, then the two modes alternate; the
median of the repetitions is reported.  The outputs of the two modes are compared byte for byte at every size that is timed.

usage: python tools/robust_bisect_probe.py [reps] [out]   -> one JSON line per case, written to profiles/robust_bisect_probe.txt"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from threshold_crypto_amd.engine import Engine, pack_messages
from threshold_crypto_amd.workload import key_set, messages

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "robust_bisect_probe.txt")
SHAPES = [(3, 10, 65536), (67, 200, 4096)]
RATES = [0.01, 1.0]
BAD_PER_JOB = [1, 3]
WORST = (67, 200, 256)
SEED = bytes(range(32))
KEY = bytes(range(64, 96))     # (a fixed key: a measurement, not a deployment)


def timed(e, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    e.sync()
    return (time.perf_counter() - t0) * 1e3, res


def world(e, dev, t, N, B):
    sks = key_set(t)
    fr = np.stack([np.frombuffer(sks.secret_key_share(i)._bytes(), dtype=np.uint8) for i in range(N)])
    flat, off = pack_messages(messages(B))
    commit = np.stack([np.frombuffer(c, dtype=np.uint8) for c in sks.public_keys(e).commit])
    d_flat, d_off = torch.from_numpy(flat).to(dev), torch.from_numpy(off.view(np.int64)).to(dev)
    d_sig, _ = e.sign(torch.from_numpy(fr).to(dev), d_flat, d_off)              # (B, N, 192): slot i = node i
    e.sync()
    return torch.from_numpy(commit).to(dev), d_sig, d_flat, d_off


def case(e, name, t, N, B, commit, s2, d_flat, d_off, n_bad_jobs, k):
    ms = {False: [], True: []}
    res, stats = {}, {}
    for rep in range(REPS + 1):                                                # the first round is the warm-up
        for mode in (False, True):
            e.set_blame_bisect(KEY if mode else None)
            dt, res[mode] = timed(e, lambda: e.combine_signatures_robust(commit, s2, msgs=d_flat, off=d_off, seed=SEED))
            stats[mode] = e.last_blame_stats()
            if rep:
                ms[mode].append(dt)
    e.set_blame_bisect(None)
    for a, b in zip(res[False][:4], res[True][:4]):
        assert bool((a == b).all().item()), name
    assert res[False][4] == res[True][4] == n_bad_jobs and int(res[True][2].sum().item()) == n_bad_jobs * k
    med = {m: float(np.median(ms[m])) for m in ms}
    row = {"case": name, "t": t, "N": N, "B": B, "bad_jobs": n_bad_jobs, "bad_shares_per_bad_job": k, "reps": REPS,
           "per_share_ms": [round(x, 2) for x in ms[False]], "bisect_ms": [round(x, 2) for x in ms[True]],
           "per_share_median_ms": round(med[False], 2), "bisect_median_ms": round(med[True], 2),
           "ratio_per_share_over_bisect": round(med[False] / med[True], 2),
           "per_share_pairing_checks": stats[False][0], "per_share_rounds": stats[False][1],
           "pairing_checks": stats[True][0], "rounds": stats[True][1]}
    return row


def main():
    e = Engine(0)
    e.set_input_checks(False)
    dev = torch.device("cuda", 0)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        with open(OUT, "w") as f:                                               # (rewritten per case: a run that is cut short keeps what it has)
            f.write("".join(json.dumps(r) + "\n" for r in rows))

    for t, N, B in SHAPES:
        commit, d_sig, d_flat, d_off = world(e, dev, t, N, B)
        for rate in RATES:
            for k in BAD_PER_JOB:
                n_bad = int(round(B * rate))
                s2 = d_sig.clone()
                js = torch.arange(0, B, B // n_bad, device=dev)[:n_bad]
                for slot in range(k):
                    s2[js, slot] = d_sig[(js + 1) % B, slot]
                emit(case(e, "rate %.2f, %d bad" % (rate, k), t, N, B, commit, s2, d_flat, d_off, n_bad, k))
                del s2
        del d_sig
        e.trim()
        torch.cuda.empty_cache()
    t, N, B = WORST
    commit, d_sig, d_flat, d_off = world(e, dev, t, N, B)
    s2 = d_sig[(torch.arange(B, device=dev) + 1) % B].contiguous()             # every share is another message's
    emit(case(e, "every share bad", t, N, B, commit, s2, d_flat, d_off, B, N))


if __name__ == "__main__":
    main()
