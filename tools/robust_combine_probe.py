"""The robust combiner (tc_combine_signatures_robust_batch) against the composition a caller had before it:
tc_verify_shares_rlc_batch over all B x N shares, ok[] read back, the first t+1 valid slots picked on the host, the shares
repacked, tc_combine_g2_batch.  Same inputs for both: shares in HBM, input checks off, every share present; a "bad job" holds
another message's share in slot 0.  The repacking of the composition is a device gather by host-made indices (the cheapest
form a caller could write).  Each timing is a host clock around calls that end in a synchronise; one warm-up of every shape,
then the two forms alternate.

usage: python tools/robust_combine_probe.py [reps]      -> one JSON line per (shape, bad-job rate), profiles/robust_combine_probe.txt"""
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


def composition(e, t, d_pks, d_sig, d_flat, d_off):
    """validate all, select on the host, repack, combine"""
    B, N = d_sig.shape[0], d_sig.shape[1]
    ok, _ = e.verify_shares_rlc(d_pks, d_sig, d_flat, d_off, seed=SEED)
    e.sync()
    ok = ok.cpu().numpy().astype(bool)
    # the first t+1 valid slots of every job (argsort keeps the order of equal keys: valid slots first, ascending)
    order = np.argsort(~ok, axis=1, kind="stable")[:, :t + 1]
    enough = ok.sum(axis=1) > t
    idx = torch.from_numpy(order.astype(np.int64)).to(d_sig.device)
    packed = torch.gather(d_sig, 1, idx[:, :, None].expand(B, t + 1, 192)).contiguous()
    sig, st = e.combine_g2(t, idx.contiguous(), packed)
    e.sync()
    return sig, st, enough


def robust(e, commit, d_sig, d_flat, d_off):
    out = e.combine_signatures_robust(commit, d_sig, msgs=d_flat, off=d_off, seed=SEED)
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
    e.set_input_checks(False)
    dev = torch.device("cuda", 0)
    for t, N, B in SHAPES:
        sks = key_set(t)
        fr = np.stack([np.frombuffer(sks.secret_key_share(i)._bytes(), dtype=np.uint8) for i in range(N)])
        flat, off = pack_messages(messages(B))
        commit = np.stack([np.frombuffer(c, dtype=np.uint8) for c in sks.public_keys(e).commit])
        pks, _ = e.public_key_shares(commit, np.arange(N, dtype=np.uint64))
        d_flat, d_off = torch.from_numpy(flat).to(dev), torch.from_numpy(off.view(np.int64)).to(dev)
        d_sig, _ = e.sign(torch.from_numpy(fr).to(dev), d_flat, d_off)          # (B, N, 192): slot i = node i
        e.sync()
        d_commit, d_pks = torch.from_numpy(commit).to(dev), torch.from_numpy(pks).to(dev)
        for rate in RATES:
            n_bad = int(round(B * rate))
            s2 = d_sig.clone()
            if n_bad:
                js = torch.arange(0, B, B // n_bad, device=dev)[:n_bad]
                s2[js, 0] = d_sig[(js + 1) % B, 0]
            ms_c, ms_r = [], []
            for rep in range(REPS + 1):                                      # the first round is the warm-up
                a, (sig_c, st_c, enough) = timed(lambda: composition(e, t, d_pks, s2, d_flat, d_off))
                b, (sig_r, used, bad, st_r, nfb) = timed(lambda: robust(e, d_commit, s2, d_flat, d_off))
                if rep:
                    ms_c.append(a)
                    ms_r.append(b)
            assert bool((sig_c == sig_r).all().item()) and not bool(st_r.any().item()) and not bool(st_c.any().item()) and enough.all()
            assert nfb == n_bad and int(bad.sum().item()) == n_bad
            row = {"t": t, "N": N, "B": B, "bad_job_rate": rate, "jobs_share_by_share": nfb, "reps": REPS,
                   "composition_ms": [round(x, 2) for x in ms_c], "robust_ms": [round(x, 2) for x in ms_r],
                   "composition_median_ms": round(float(np.median(ms_c)), 2), "robust_median_ms": round(float(np.median(ms_r)), 2),
                   "ratio_composition_over_robust": round(float(np.median(ms_c) / np.median(ms_r)), 2)}
            print(json.dumps(row), flush=True)
        del d_sig, s2
        e.trim()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
