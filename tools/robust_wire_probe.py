"""The wire-level robust combiner (tc_combine_signatures_robust_wire_batch) against the composition a caller had before it:
tc_g2_decompress_batch of all B x N compressed shares, tc_combine_signatures_robust_batch, tc_g2_compress_batch of the
results.  Same inputs for both: compressed shares in HBM, input checks ON (what the wire form always applies to its shares),
every share present; a "bad job" holds another message's share in slot 0.  Each timing is a host clock around calls that end
in a synchronise; one warm-up of every shape, then the two forms alternate.  Equal outputs are asserted.

usage: python tools/robust_wire_probe.py [reps]      -> one JSON line per (shape, bad-job rate), profiles/robust_wire_probe.txt"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from threshold_crypto_amd.engine import Engine, pack_messages
from threshold_crypto_amd.workload import key_set, messages

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
SHAPES = [(3, 10, 65536), (67, 200, 4096)]
RATES = [0.0, 0.01, 1.0]
SEED = bytes(range(32))


def composition(e, commit, d_wire, d_flat, d_off):
    """decompress everything, the uncompressed robust entry, compress the results"""
    B, N = d_wire.shape[0], d_wire.shape[1]
    full, _ = e.g2_decompress(d_wire.reshape(B * N, 96))
    sig, used, bad, st, nfb = e.combine_signatures_robust(commit, full.reshape(B, N, 192), msgs=d_flat, off=d_off, seed=SEED)
    out, _ = e.g2_compress(sig)
    e.sync()
    return out, used, bad, st, nfb


def wire(e, commit, d_wire, d_flat, d_off):
    out = e.combine_signatures_robust_wire(commit, d_wire, msgs=d_flat, off=d_off, seed=SEED)
    e.sync()
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def main():
    e = Engine(0)
    dev = torch.device("cuda", 0)
    for t, N, B in SHAPES:
        sks = key_set(t)
        fr = np.stack([np.frombuffer(sks.secret_key_share(i)._bytes(), dtype=np.uint8) for i in range(N)])
        flat, off = pack_messages(messages(B))
        commit = np.stack([np.frombuffer(c, dtype=np.uint8) for c in sks.public_keys(e).commit])
        d_flat, d_off = torch.from_numpy(flat).to(dev), torch.from_numpy(off.view(np.int64)).to(dev)
        d_sig, _ = e.sign(torch.from_numpy(fr).to(dev), d_flat, d_off)          # (B, N, 192): slot i = node i
        d_wire, _ = e.g2_compress(d_sig.reshape(B * N, 192))
        e.sync()
        d_wire = d_wire.reshape(B, N, 96)
        del d_sig
        d_commit = torch.from_numpy(commit).to(dev)
        for rate in RATES:
            n_bad = int(round(B * rate))
            s2 = d_wire.clone()
            if n_bad:
                js = torch.arange(0, B, B // n_bad, device=dev)[:n_bad]
                s2[js, 0] = d_wire[(js + 1) % B, 0]
            ms_c, ms_w = [], []
            for rep in range(REPS + 1):                                      # the first round is the warm-up
                a, (sig_c, used_c, bad_c, st_c, nfb_c) = timed(lambda: composition(e, d_commit, s2, d_flat, d_off))
                b, (sig_w, used_w, bad_w, st_w, nfb_w) = timed(lambda: wire(e, d_commit, s2, d_flat, d_off))
                if rep:
                    ms_c.append(a)
                    ms_w.append(b)
            assert bool((sig_c == sig_w).all().item()) and bool((used_c == used_w).all().item()) and bool((bad_c == bad_w).all().item())
            assert not bool(st_w.any().item()) and not bool(st_c.any().item())
            assert nfb_w == n_bad and nfb_c == n_bad and int(bad_w.sum().item()) == n_bad
            row = {"t": t, "N": N, "B": B, "bad_job_rate": rate, "jobs_share_by_share": nfb_w, "reps": REPS,
                   "composition_ms": [round(x, 2) for x in ms_c], "wire_ms": [round(x, 2) for x in ms_w],
                   "composition_median_ms": round(float(np.median(ms_c)), 2), "wire_median_ms": round(float(np.median(ms_w)), 2),
                   "ratio_composition_over_wire": round(float(np.median(ms_c) / np.median(ms_w)), 2)}
            print(json.dumps(row), flush=True)
        del d_wire, s2
        e.trim()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
