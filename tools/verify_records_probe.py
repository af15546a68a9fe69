"""Batch verification of ragged input (tc_verify_g2_records_rlc_batch) against the paths that take the same
operands without it: tc_verify_g2_batch with pk_stride = 96 on the expanded arrays and, where the shape is dense,
tc_verify_shares_rlc_batch.  Device-resident operands, one MI355X; per shape and path `reps` timed calls after a warm-up, HIP-event
time (tc_last_kernel_ms: first launch to last kernel of the call, the entry's own host round trips included) and wall time,
min / median.  Every timed result is compared with the per-record path's.

usage: python tools/verify_records_probe.py [--out profiles/verify_records_probe.txt] [--reps 7] [--label <commit>] [--small]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from threshold_crypto_amd.engine import Engine, pack_messages

R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "verify_records_probe.txt"))
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--label", default="unknown")
ap.add_argument("--small", action="store_true", help="a sixteenth of every shape (a quick look, not a measurement)")
args = ap.parse_args()
SCALE = 16 if args.small else 1

e = Engine(0)
e.set_timing(True)
dev = torch.device("cuda", 0)
rng = np.random.default_rng(20261019)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def fr_rows(n):
    """n fixed non-zero scalars below r"""
    out = np.zeros((n, 32), dtype=np.uint8)
    for i in range(n):
        out[i] = np.frombuffer(((0x9E3779B97F4A7C15 * (i + 1) ** 3 + 12345) % R_MOD).to_bytes(32, "little"), dtype=np.uint8)
    return out


def t8(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)


def timed(call):
    """(event ms, wall ms) lists over args.reps calls after one warm-up, and the last result"""
    call()
    e.sync()
    ev, wall, res = [], [], None
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call()
        e.sync()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(e.last_kernel_ms())
    return ev, wall, res


def fmt(ev, wall, R):
    return "event min %8.2f med %8.2f ms | wall min %8.2f med %8.2f ms | %6.2f M records/s (event min)" % (
        min(ev), statistics.median(ev), min(wall), statistics.median(wall), R / min(ev) / 1e3)


def run_shape(name, pks, key_idx, sigs, rec_off, msgs, dense=None, checked=True):
    """pks (K, 96), key_idx (R,), sigs (R, 192), rec_off (M + 1,): numpy; msgs: list of bytes; dense = (B, N) when every record is present"""
    M, R, Kn = len(msgs), sigs.shape[0], pks.shape[0]
    flat, off = pack_messages(msgs)
    d_flat, d_off = t8(flat), t64(off)
    d_hash = e.hash_g2(d_flat, d_off)
    msg_of = np.repeat(np.arange(M), np.diff(rec_off.astype(np.int64)))
    d_pks, d_kidx, d_sigs, d_rec = t8(pks), t64(key_idx), t8(sigs), t64(rec_off)
    d_pk_x = d_pks[torch.from_numpy(key_idx.astype(np.int64)).to(dev)].contiguous()
    d_hash_x = d_hash[torch.from_numpy(msg_of).to(dev)].contiguous()
    e.set_input_checks(checked)
    say("## %s: M = %d messages, R = %d records, K = %d keys, input checks %s" % (name, M, R, Kn, "on" if checked else "off"))
    ev0, wall0, ok_ref = timed(lambda: e.verify_g2(d_pk_x, d_sigs, d_hash_x))
    say("  per-record  tc_verify_g2_batch (pk_stride 96, expanded)   %s" % fmt(ev0, wall0, R))
    n_bad = int((ok_ref == 0).sum().item())
    out = {"name": name, "M": M, "R": R, "K": Kn, "checked": checked, "rejected": n_bad, "per_record_ms": min(ev0)}
    seed = bytes(range(32))
    ev, wall, (ok, nfb) = timed(lambda: e.verify_g2_records_rlc(d_pks, d_kidx, d_sigs, d_rec, d_hash, seed=seed))
    assert bool((ok == ok_ref).all().item()), "records entry differs from the per-record path"
    say("  ragged      tc_verify_g2_records_rlc_batch (pre-hashed)    %s | n_fallback %d | x%.2f vs per-record" % (fmt(ev, wall, R), nfb, min(ev0) / min(ev)))
    out.update(records_ms=min(ev), n_fallback=nfb, speedup=min(ev0) / min(ev))
    ev, wall, (ok, nfb) = timed(lambda: e.verify_sig_records_rlc(d_pks, d_kidx, d_sigs, d_rec, d_flat, d_off, seed=seed))
    assert bool((ok == ok_ref).all().item())
    say("  ragged      tc_verify_sig_records_rlc_batch (hashing)      %s" % fmt(ev, wall, R))
    out.update(records_sig_ms=min(ev))
    if dense:
        B, N = dense
        d_sh = d_sigs.reshape(B, N, 192)
        ev, wall, (okm, nfm) = timed(lambda: e.verify_shares_rlc(d_pks, d_sh, d_flat, d_off, seed=seed))
        assert bool((okm.reshape(-1) == ok_ref).all().item())
        say("  dense       tc_verify_shares_rlc_batch (hashing)           %s | messages in fallback %d | ragged (hashing) / dense = %.2f" % (
            fmt(ev, wall, R), nfm, out["records_sig_ms"] / min(ev)))
        out.update(shares_rlc_ms=min(ev))
    e.set_input_checks(True)
    say("")
    return out


def key_table(n):
    sk = fr_rows(n)
    pks, st = e.g1_commitment(sk)
    assert not np.asarray(st).any()
    return sk, np.ascontiguousarray(pks)


def dense_world(N, B):
    """every signature sk_i H_m: (B, N, 192)"""
    sk, pks = key_table(N)
    msgs = [b"probe message %d" % m for m in range(B)]
    flat, off = pack_messages(msgs)
    hashes = e.hash_g2(flat, off)
    sig, st = e.g2_mul(sk, hashes)
    assert not np.asarray(st).any()
    return pks, msgs, np.ascontiguousarray(sig)


say("# verify_records_probe: %s, commit %s, %d timed calls per line after one warm-up%s" % (e.version(), args.label, args.reps, ", SMALL shapes" if args.small else ""))
say("# torch %s, device %s" % (torch.__version__, torch.cuda.get_device_name(0)))
say("")
results = []
for checked in (True, False):
    # dense N = 10 x 6 553 messages, the same with 30 % of the records dropped, and with 1 % of the messages holding a forged record
    N, B = 10, 6553 // SCALE
    pks, msgs, sig = dense_world(N, B)
    kidx = np.tile(np.arange(N, dtype=np.uint64), B)
    rec_off = np.arange(B + 1, dtype=np.uint64) * N
    flat_sig = sig.reshape(B * N, 192)
    results.append(run_shape("dense N = 10", pks, kidx, flat_sig, rec_off, msgs, dense=(B, N), checked=checked))
    keep = rng.random(B * N) >= 0.3
    lens = keep.reshape(B, N).sum(axis=1)
    off_s = np.zeros(B + 1, dtype=np.uint64)
    off_s[1:] = np.cumsum(lens)
    results.append(run_shape("sparse N = 10, 30 % dropped", pks, kidx[keep], np.ascontiguousarray(flat_sig[keep]), off_s, msgs, checked=checked))
    forged = flat_sig.copy()
    bad_msgs = rng.choice(B, size=max(1, B // 100), replace=False)
    for m in bad_msgs:
        forged[m * N + 3] = flat_sig[m * N + 4]                     # node 3 sends node 4's share
    results.append(run_shape("dense N = 10, 1 % of the messages forged", pks, kidx, forged, rec_off, msgs, dense=(B, N), checked=checked))
    del sig, flat_sig, forged
    # N = 200 x 328 messages
    N, B = 200, max(1, 328 // SCALE)
    pks, msgs, sig = dense_world(N, B)
    results.append(run_shape("dense N = 200", pks, np.tile(np.arange(N, dtype=np.uint64), B), sig.reshape(B * N, 192), np.arange(B + 1, dtype=np.uint64) * N, msgs,
                             dense=(B, N), checked=checked))
    del sig
    # M = R = 65 536 unrelated triples, distinct keys
    n = 65536 // SCALE
    sk, pks = key_table(n)
    msgs = [b"unrelated %d" % m for m in range(n)]
    flat, off = pack_messages(msgs)
    hashes = e.hash_g2(flat, off)
    sig, st = e.sign_shares_g2(sk, np.arange(n, dtype=np.uint64)[:, None].copy(), hashes)
    assert not np.asarray(st).any()
    results.append(run_shape("unrelated triples", pks, np.arange(n, dtype=np.uint64), np.ascontiguousarray(sig[:, 0]), np.arange(n + 1, dtype=np.uint64), msgs,
                             checked=checked))
    del sig
say("# json " + json.dumps(results))
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
