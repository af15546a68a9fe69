"""Decryption-share verification of ragged input (tc_verify_decryption_share_records_rlc_batch) against the
paths that take the same operands without it: tc_verify_decryption_share_batch with pk_stride = 96 on the expanded arrays and,
where the shape is dense, tc_verify_decryption_shares_rlc_batch.  Device-resident operands, one MI355X; per shape and path `reps`
timed calls after a warm-up, HIP-event time (tc_last_kernel_ms: first launch to last kernel of the call, the entry's own host
round trips included) and wall time, min / median.  Every timed result is compared with the per-record path's.

Measured (profiles/dshare_records_probe.txt, at about 65 536 records, event min, input checks on / off), the hashing ragged entry
against the per-record path: 1.41x / 1.60x dense at 10 keys x 6 553 ciphertexts, 1.28x / 1.53x with 30 % of those records
dropped, 1.91x / 2.40x at 200 keys x 328 ciphertexts; SLOWER with a forged record in 1 % of the ciphertexts, 0.80x / 0.92x, and
level for 65 536 unrelated triples, 0.95x / 1.00x.  Against the dense entry on dense input it is slower: 0.79x / 0.95x at 10
keys, 0.80x / 0.96x at 200 keys, 0.78x / 0.83x with the forged records.

usage: python tools/dshare_records_probe.py [--out profiles/dshare_records_probe.txt] [--reps 7] [--label <commit>] [--small]
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
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dshare_records_probe.txt"))
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--label", default="unknown")
ap.add_argument("--small", action="store_true", help="a sixteenth of every shape (a quick look, not a measurement)")
args = ap.parse_args()
SCALE = 16 if args.small else 1

e = Engine(0)
e.set_timing(True)
dev = torch.device("cuda", 0)
rng = np.random.default_rng(20261020)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def scalars(n, salt):
    """n fixed non-zero scalars below r"""
    return [(0x9E3779B97F4A7C15 * (i + 1) ** 3 + salt) % R_MOD for i in range(n)]


def fr_rows(vals):
    out = np.zeros((len(vals), 32), dtype=np.uint8)
    for i, v in enumerate(vals):
        out[i] = np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)
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


VLEN = 32  # bytes of every ciphertext's v


def run_shape(name, pks, key_idx, shares, rec_off, cts, dense=None, checked=True):
    """pks (K, 96), key_idx (R,), shares (R, 96), rec_off (M + 1,), cts = (u (M, 96), v (M * VLEN,), w (M, 192)): numpy; dense = (B, N) when
    every record is present"""
    u, v, w = cts
    M, R, Kn = u.shape[0], shares.shape[0], pks.shape[0]
    off = np.arange(M + 1, dtype=np.uint64) * VLEN
    d_u, d_v, d_off, d_w = t8(u), t8(v), t64(off), t8(w)
    d_hash, st = e.hash_g1_g2(d_u, d_v, d_off)
    ct_of = torch.from_numpy(np.repeat(np.arange(M), np.diff(rec_off.astype(np.int64)))).to(dev)
    d_pks, d_kidx, d_sh, d_rec = t8(pks), t64(key_idx), t8(shares), t64(rec_off)
    d_pk_x = d_pks[torch.from_numpy(key_idx.astype(np.int64)).to(dev)].contiguous()
    d_u_x, d_w_x = d_u[ct_of].contiguous(), d_w[ct_of].contiguous()
    d_v_x = d_v.reshape(M, VLEN)[ct_of].contiguous().reshape(-1)
    d_off_x = t64(np.arange(R + 1, dtype=np.uint64) * VLEN)
    e.set_input_checks(checked)
    say("## %s: M = %d ciphertexts, R = %d records, K = %d keys, input checks %s" % (name, M, R, Kn, "on" if checked else "off"))
    ev0, wall0, ok_ref = timed(lambda: e.verify_decryption_share(d_pk_x, d_sh, d_u_x, d_v_x, d_off_x, d_w_x))
    say("  per-record  tc_verify_decryption_share_batch (pk_stride 96, expanded)          %s" % fmt(ev0, wall0, R))
    n_bad = int((ok_ref == 0).sum().item())
    out = {"name": name, "M": M, "R": R, "K": Kn, "checked": checked, "rejected": n_bad, "per_record_ms": min(ev0)}
    seed = bytes(range(32))
    ev, wall, (ok, nfb) = timed(lambda: e.verify_decryption_share_records_rlc(d_pks, d_kidx, d_sh, d_rec, d_u, d_v, d_off, d_w, seed=seed))
    assert bool((ok == ok_ref).all().item()), "records entry differs from the per-record path"
    say("  ragged      tc_verify_decryption_share_records_rlc_batch (hashing)             %s | n_fallback %d | x%.2f vs per-record" % (
        fmt(ev, wall, R), nfb, min(ev0) / min(ev)))
    out.update(records_ms=min(ev), n_fallback=nfb, speedup=min(ev0) / min(ev))
    ev, wall, (ok, nfb) = timed(lambda: e.verify_decryption_share_records_prehashed_rlc(d_pks, d_kidx, d_sh, d_rec, d_hash, d_w, seed=seed))
    assert bool((ok == ok_ref).all().item()), "pre-hashed records entry differs from the per-record path"
    say("  ragged      tc_verify_decryption_share_records_prehashed_rlc_batch             %s | x%.2f vs per-record (which hashes)" % (
        fmt(ev, wall, R), min(ev0) / min(ev)))
    out.update(records_prehashed_ms=min(ev))
    if dense:
        B, N = dense
        d_mat = d_sh.reshape(B, N, 96)
        ev, wall, (okm, nfm) = timed(lambda: e.verify_decryption_shares_rlc(d_pks, d_mat, d_u, d_v, d_off, d_w, seed=seed))
        assert bool((okm.reshape(-1) == ok_ref).all().item())
        say("  dense       tc_verify_decryption_shares_rlc_batch (hashing)                    %s | ciphertexts in fallback %d | x%.2f ragged (hashing) vs dense" % (
            fmt(ev, wall, R), nfm, min(ev) / out["records_ms"]))
        out.update(shares_rlc_ms=min(ev), speedup_vs_dense=min(ev) / out["records_ms"])
    e.set_input_checks(True)
    say("")
    return out


def key_table(n, salt):
    sk = scalars(n, salt)
    pks, st = e.g1_commitment(fr_rows(sk))
    assert not np.asarray(st).any()
    return sk, np.ascontiguousarray(pks)


def ciphertexts(B, salt):
    """B ciphertexts of VLEN-byte plaintexts under one master key, with their encryption scalars"""
    _, master = key_table(1, 777)
    r = scalars(B, salt)
    plain = rng.integers(0, 256, size=B * VLEN, dtype=np.uint8)
    u, v, w, st = e.encrypt(np.ascontiguousarray(master[0]), fr_rows(r), plain, np.arange(B + 1, dtype=np.uint64) * VLEN)
    assert not np.asarray(st).any()
    return r, (np.ascontiguousarray(u), np.ascontiguousarray(v), np.ascontiguousarray(w))


def dense_world(N, B):
    """every share sk_i u_c: (B, N, 96)"""
    sk, pks = key_table(N, 12345)
    _, cts = ciphertexts(B, 999)
    sh, st = e.g1_mul(fr_rows(sk), cts[0])
    assert not np.asarray(st).any()
    return pks, cts, np.ascontiguousarray(sh)


say("# dshare_records_probe: %s, commit %s, %d timed calls per line after one warm-up%s" % (e.version(), args.label, args.reps, ", SMALL shapes" if args.small else ""))
say("# torch %s, device %s" % (torch.__version__, torch.cuda.get_device_name(0)))
say("")
results = []
for checked in (True, False):
    # dense N = 10 x 6 553 ciphertexts, the same with 30 % of the records dropped, and with 1 % of the ciphertexts holding a forged record
    N, B = 10, 6553 // SCALE
    pks, cts, sh = dense_world(N, B)
    kidx = np.tile(np.arange(N, dtype=np.uint64), B)
    rec_off = np.arange(B + 1, dtype=np.uint64) * N
    flat_sh = sh.reshape(B * N, 96)
    results.append(run_shape("dense N = 10", pks, kidx, flat_sh, rec_off, cts, dense=(B, N), checked=checked))
    keep = rng.random(B * N) >= 0.3
    lens = keep.reshape(B, N).sum(axis=1)
    off_s = np.zeros(B + 1, dtype=np.uint64)
    off_s[1:] = np.cumsum(lens)
    results.append(run_shape("sparse N = 10, 30 % dropped", pks, kidx[keep], np.ascontiguousarray(flat_sh[keep]), off_s, cts, checked=checked))
    forged = flat_sh.copy()
    bad_cts = rng.choice(B, size=max(1, B // 100), replace=False)
    for m in bad_cts:
        forged[m * N + 3] = flat_sh[m * N + 4]                      # node 3 sends node 4's share
    results.append(run_shape("dense N = 10, 1 % of the ciphertexts forged", pks, kidx, forged, rec_off, cts, dense=(B, N), checked=checked))
    del sh, flat_sh, forged
    # N = 200 x 328 ciphertexts
    N, B = 200, max(1, 328 // SCALE)
    pks, cts, sh = dense_world(N, B)
    results.append(run_shape("dense N = 200", pks, np.tile(np.arange(N, dtype=np.uint64), B), sh.reshape(B * N, 96), np.arange(B + 1, dtype=np.uint64) * N, cts,
                             dense=(B, N), checked=checked))
    del sh
    # M = R = 65 536 unrelated triples, distinct keys: share_i = sk_i u_i = [sk_i r_i] g1
    n = 65536 // SCALE
    sk, pks = key_table(n, 12345)
    r, cts = ciphertexts(n, 4242)
    sh, st = e.g1_commitment(fr_rows([a * b % R_MOD for a, b in zip(sk, r)]))
    assert not np.asarray(st).any()
    results.append(run_shape("unrelated triples", pks, np.arange(n, dtype=np.uint64), np.ascontiguousarray(sh), np.arange(n + 1, dtype=np.uint64), cts,
                             checked=checked))
    del sh
say("# json " + json.dumps(results))
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
