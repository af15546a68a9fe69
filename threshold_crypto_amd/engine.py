"""Engine: one context of libtc_amd.so bound to one MI355X, with array-level batch calls.

Arrays are either numpy (host memory: the library stages through its own device buffers)
or torch CUDA tensors (device-resident: nothing crosses PCIe; torch is used only as the
owner of device memory).  All compute happens in the HIP kernels behind the C ABI.
"""
import ctypes

import numpy as np

from . import _native

G1_BYTES = 96
G2_BYTES = 192
FR_BYTES = 32


class TcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libtc_amd call failed (%d): %s" % (code, msg))
        self.code = code


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _ptr(x):
    if x is None:
        return None
    if _is_torch(x):
        return ctypes.c_void_p(x.data_ptr())
    return ctypes.c_void_p(x.ctypes.data)


def pack_messages(msgs):
    """list of bytes -> (flat uint8 array, uint64 offsets[B+1])"""
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    if len(msgs):
        off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    flat = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy() if len(msgs) else np.zeros(0, np.uint8)
    if flat.size == 0:
        flat = np.zeros(1, np.uint8)
    return flat, off


class Engine:
    """Owns a tc_ctx.  Raises if the native library or a HIP device is missing."""

    def __init__(self, device=0):
        self._lib = _native.load()
        ctx = ctypes.c_void_p()
        rc = self._lib.tc_ctx_create(ctypes.byref(ctx), int(device))
        if rc != _native.TC_OK:
            raise TcError(rc, "tc_ctx_create failed on device %d (no gfx950 HIP device? there is no CPU fallback)"
                          % device)
        self._ctx = ctx
        self.device = int(device)
        self._device_io = False
        # device-I/O calls return before their kernels have run: the operand tensors of the calls since the last sync() are
        # kept alive here, so that `eng.verify_sig(pk.to(dev), ...)` with temporaries is not a use-after-free (torch would hand a
        # dead tensor's memory to the next allocation while the kernels still read it)
        self._keep = {}

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.tc_ctx_destroy(self._ctx)     # (waits for the context's streams)
            self._ctx = None
            self._keep.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing ---------------------------------------------------------------------------
    def set_timing(self, on):
        self._lib.tc_ctx_set_timing(self._ctx, 1 if on else 0)

    def set_input_checks(self, on):
        """checked-input mode (the context's default): every point operand is tested for order-r membership on the
        device first.  False is the explicit opt-out for operands known to be members (this library's own outputs)."""
        self._lib.tc_ctx_set_input_checks(self._ctx, 1 if on else 0)

    def input_checks(self):
        return bool(self._lib.tc_ctx_get_input_checks(self._ctx))

    def set_blame_bisect(self, key=None):
        """Pass 2 of the four robust combiners (tc_ctx_set_blame_bisect): None = one pairing check per present share (the
        default); 32 secret random bytes = blame by bisection -- range checks over shares multiplied by secret scalars, at most
        min(1 + 2 k d, 2 N - 1) checks for a job with k bad shares among N (d = ceil(log2 N)), the same outputs up to 2^-63 per
        check.  The key must stay secret for the context's lifetime; every call derives scalars of its own from it."""
        if key is not None:
            key = bytes(key)
            if len(key) != 32:
                raise ValueError("key: 32 bytes")
        rc = self._lib.tc_ctx_set_blame_bisect(self._ctx, key)
        if rc != 0:
            raise TcError(rc, "tc_ctx_set_blame_bisect")

    def blame_bisect(self):
        return bool(self._lib.tc_ctx_get_blame_bisect(self._ctx))

    def last_blame_stats(self):
        """(pairing checks, rounds) pass 2 of the last robust call on this context spent: F * N and 1 share by share for F
        messages examined, the search's totals by bisection, (0, 0) when no message reached pass 2"""
        checks, rounds = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = self._lib.tc_ctx_last_blame_stats(self._ctx, ctypes.byref(checks), ctypes.byref(rounds))
        if rc != 0:
            raise TcError(rc, "tc_ctx_last_blame_stats")
        return int(checks.value), int(rounds.value)

    def trim(self):
        """give the context's staging / table buffers back to the device (tc_ctx_trim)"""
        self._lib.tc_ctx_trim(self._ctx)

    def transfer_bytes(self):
        """(host-to-device, device-to-host) bytes this context's staging copies have moved over PCIe"""
        up, down = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._lib.tc_ctx_transfer_bytes(self._ctx, ctypes.byref(up), ctypes.byref(down))
        return int(up.value), int(down.value)

    def tuning(self):
        """the form choices of this context (tc_ctx_get_tuning): jobs from which a checked G2 decode / a hash takes two jobs per
        lane pair, the pairing form (0 = by batch size), the line-buffer budget (0 = a third of the free HBM), whether the membership
        tests of checked-input mode run beside the main kernels on a second stream.  Fixed when the context was created (defaults, or
        TC_DUO_MIN / TC_PAIRING_FORM / TC_PAIRING_BUDGET / TC_CHECKS_BESIDE / TC_MSM_BUDGET / TC_PRIVATE_RESERVE in the environment at that
        moment)."""
        out = (ctypes.c_uint64 * 8)()
        rc = self._lib.tc_ctx_get_tuning(self._ctx, out)
        if rc != 0:
            raise TcError(rc, "tc_ctx_get_tuning")
        return {"duo_min_decode": int(out[0]), "duo_min_hash": int(out[1]), "pairing_form": int(out[2]), "pairing_budget": int(out[3]),
                "checks_beside": int(out[4]), "msm_budget": int(out[5]), "private_reserve": int(out[6])}

    def last_kernel_ms(self):
        return float(self._lib.tc_last_kernel_ms(self._ctx))

    def set_stream(self, stream_ptr):
        self._lib.tc_ctx_set_stream(self._ctx, ctypes.c_void_p(stream_ptr) if stream_ptr else None)

    def sync(self):
        self._lib.tc_sync(self._ctx)
        self._keep.clear()

    def version(self):
        return self._lib.tc_version().decode()

    def _mode(self, *arrays):
        dev = [a for a in arrays if a is not None and _is_torch(a)]
        if dev and len(dev) != len([a for a in arrays if a is not None]):
            raise ValueError("mixing host (numpy) and device (torch) arrays in one call")
        want = bool(dev)
        for a in dev:
            self._keep[id(a)] = a
        if want != self._device_io:
            self._lib.tc_ctx_set_device_io(self._ctx, 1 if want else 0)
            self._device_io = want
        return want

    def _empty(self, like_device, shape, dtype=np.uint8, ref=None):
        if like_device:
            import torch
            tdt = {np.uint8: torch.uint8, np.uint64: torch.int64}[dtype]
            return torch.empty(shape, dtype=tdt, device=ref.device)
        return np.empty(shape, dtype=dtype)

    def _call(self, name, *args):
        rc = getattr(self._lib, name)(self._ctx, *args)
        if rc != _native.TC_OK:
            raise TcError(rc, self._lib.tc_last_error(self._ctx).decode())

    @staticmethod
    def _arg(a, shape, kind, name):
        """Every operand is validated before its raw pointer crosses the C ABI: dtype (`kind` "u8" or
        "u64"), C-contiguity and the FULL expected shape (None = any extent).  A wrong dtype or a sliced
        view would otherwise be misread, or read out of bounds, by the library."""
        if a is None:
            raise ValueError("%s is required" % name)
        torch_arr = _is_torch(a)
        dt = str(a.dtype)
        good = {"u8": ("uint8", "torch.uint8"), "u64": ("uint64", "int64", "torch.int64", "torch.uint64")}[kind]
        if dt not in good:
            raise TypeError("%s: expected dtype %s, got %s" % (name, good[0], dt))
        if len(a.shape) != len(shape) or any(w is not None and int(g) != int(w) for g, w in zip(a.shape, shape)):
            raise ValueError("%s: expected shape %s, got %s" % (name, tuple(shape), tuple(a.shape)))
        if not (a.is_contiguous() if torch_arr else a.flags["C_CONTIGUOUS"]):
            raise ValueError("%s must be C-contiguous" % name)
        return a

    def _msgs(self, msgs, off, B=None):
        """a message blob + its offsets[B+1]; returns B"""
        self._arg(off, (None,), "u64", "off")
        if off.shape[0] < 1:
            raise ValueError("off must hold B+1 entries")
        if B is not None and off.shape[0] != B + 1:
            raise ValueError("off holds %d entries for %d jobs (expected B+1)" % (off.shape[0], B))
        self._arg(msgs, (None,), "u8", "msgs")
        return off.shape[0] - 1

    def _point(self, a, nbytes, B, name):
        """a per-job (B, nbytes) operand or ONE (nbytes,) operand broadcast to every job; returns the stride"""
        if len(a.shape) == 1:
            self._arg(a, (nbytes,), "u8", name)
            return 0
        self._arg(a, (B, nbytes), "u8", name)
        return nbytes

    # -- hashing ------------------------------------------------------------------------------
    def hash_g2(self, msgs, off):
        dev = self._mode(msgs, off)
        B = self._msgs(msgs, off)
        out = self._empty(dev, (B, G2_BYTES), ref=msgs)
        self._call("tc_hash_g2_batch", _ptr(msgs), _ptr(off), B, _ptr(out))
        return out

    def hash_g1_g2(self, g1, msgs, off):
        dev = self._mode(g1, msgs, off)
        B = self._msgs(msgs, off)
        self._arg(g1, (B, G1_BYTES), "u8", "g1")
        out = self._empty(dev, (B, G2_BYTES), ref=g1)
        st = self._empty(dev, (B,), ref=g1)
        self._call("tc_hash_g1_g2_batch", _ptr(g1), _ptr(msgs), _ptr(off), B, _ptr(out), _ptr(st))
        return out, st

    # -- scalar multiplication -------------------------------------------------------------------
    def _mul(self, name, pb, fr, pts):
        dev = self._mode(fr, pts)
        self._arg(fr, (None, FR_BYTES), "u8", "fr")
        self._arg(pts, (None, pb), "u8", "pts")
        S, B = fr.shape[0], pts.shape[0]
        out = self._empty(dev, (B, S, pb), ref=pts)
        st = self._empty(dev, (B, S), ref=pts)
        self._call(name, _ptr(fr), _ptr(pts), S, B, _ptr(out), _ptr(st))
        return out, st

    def g2_mul(self, fr, pts):
        """out[j, s] = fr[s] * pts[j]"""
        return self._mul("tc_g2_mul_batch", G2_BYTES, fr, pts)

    def g1_mul(self, fr, pts):
        return self._mul("tc_g1_mul_batch", G1_BYTES, fr, pts)

    def sign_shares_g2(self, sk_table, idx, hashes):
        """out[j, k] = sk_table[idx[j, k]] * hashes[j]: the shares of each message by its selected signers"""
        dev = self._mode(sk_table, idx, hashes)
        self._arg(sk_table, (None, FR_BYTES), "u8", "sk_table")
        self._arg(idx, (None, None), "u64", "idx")
        B, n = idx.shape
        self._arg(hashes, (B, G2_BYTES), "u8", "hashes")
        out = self._empty(dev, (B, n, G2_BYTES), ref=hashes)
        st = self._empty(dev, (B, n), ref=hashes)
        self._call("tc_sign_shares_g2_batch", _ptr(sk_table), sk_table.shape[0], _ptr(idx), _ptr(hashes), n, B, _ptr(out), _ptr(st))
        return out, st

    def decrypt_shares_g1(self, sk_table, idx, u):
        """out[j, k] = sk_table[idx[j, k]] * u[j]: SecretKeyShare::decrypt_share_no_verify (src/lib.rs:460-462) for the selected
        holders of each ciphertext -> (shares (B, n, 96), status (B, n))"""
        dev = self._mode(sk_table, idx, u)
        self._arg(sk_table, (None, FR_BYTES), "u8", "sk_table")
        self._arg(idx, (None, None), "u64", "idx")
        B, n = idx.shape
        self._arg(u, (B, G1_BYTES), "u8", "u")
        out = self._empty(dev, (B, n, G1_BYTES), ref=u)
        st = self._empty(dev, (B, n), ref=u)
        self._call("tc_decrypt_shares_g1_batch", _ptr(sk_table), sk_table.shape[0], _ptr(idx), _ptr(u), n, B, _ptr(out), _ptr(st))
        return out, st

    def sign(self, fr, msgs, off):
        dev = self._mode(fr, msgs, off)
        self._arg(fr, (None, FR_BYTES), "u8", "fr")
        S, B = fr.shape[0], self._msgs(msgs, off)
        out = self._empty(dev, (B, S, G2_BYTES), ref=fr)
        st = self._empty(dev, (B, S), ref=fr)
        self._call("tc_sign_batch", _ptr(fr), _ptr(msgs), _ptr(off), S, B, _ptr(out), _ptr(st))
        return out, st

    # -- combination --------------------------------------------------------------------------------
    def _combine(self, name, pb, t, idx, shares):
        dev = self._mode(idx, shares)
        self._arg(idx, (None, None), "u64", "idx")
        B, n = idx.shape
        self._arg(shares, (B, n, pb), "u8", "shares")
        out = self._empty(dev, (B, pb), ref=shares)
        st = self._empty(dev, (B,), ref=shares)
        self._call(name, int(t), int(n), _ptr(idx), _ptr(shares), B, _ptr(out), _ptr(st))
        return out, st

    def combine_g2(self, t, idx, shares):
        return self._combine("tc_combine_g2_batch", G2_BYTES, t, idx, shares)

    def combine_g1(self, t, idx, shares):
        return self._combine("tc_combine_g1_batch", G1_BYTES, t, idx, shares)

    def _combine_fr(self, name, pb, t, idx_fr, shares):
        """`T: IntoFr` abscissae as (B, n, 32) little-endian Fr values (src/into_fr.rs)"""
        dev = self._mode(idx_fr, shares)
        self._arg(idx_fr, (None, None, FR_BYTES), "u8", "idx_fr")
        B, n = idx_fr.shape[0], idx_fr.shape[1]
        self._arg(shares, (B, n, pb), "u8", "shares")
        out = self._empty(dev, (B, pb), ref=shares)
        st = self._empty(dev, (B,), ref=shares)
        self._call(name, int(t), int(n), _ptr(idx_fr), _ptr(shares), B, _ptr(out), _ptr(st))
        return out, st

    def combine_g2_fr(self, t, idx_fr, shares):
        return self._combine_fr("tc_combine_g2_fr_batch", G2_BYTES, t, idx_fr, shares)

    def combine_g1_fr(self, t, idx_fr, shares):
        return self._combine_fr("tc_combine_g1_fr_batch", G1_BYTES, t, idx_fr, shares)

    def combine_signatures_wire(self, t, idx, shares96):
        """PublicKeySet::combine_signatures on the wire forms: (B, n, 96) compressed shares in (checked decode of from_bytes on
        the device), (B, 96) Signature::to_bytes out"""
        dev = self._mode(idx, shares96)
        self._arg(idx, (None, None), "u64", "idx")
        B, n = idx.shape
        self._arg(shares96, (B, n, G2_BYTES // 2), "u8", "shares96")
        out = self._empty(dev, (B, G2_BYTES // 2), ref=shares96)
        st = self._empty(dev, (B,), ref=shares96)
        self._call("tc_combine_signatures_wire_batch", int(t), int(n), _ptr(idx), _ptr(shares96), B, _ptr(out), _ptr(st))
        return out, st

    def _lincomb(self, name, pb, scalars, points):
        dev = self._mode(scalars, points)
        self._arg(scalars, (None, None, FR_BYTES), "u8", "scalars")
        B, n = scalars.shape[0], scalars.shape[1]
        self._arg(points, (B, n, pb), "u8", "points")
        out = self._empty(dev, (B, pb), ref=points)
        st = self._empty(dev, (B,), ref=points)
        self._call(name, int(n), _ptr(scalars), _ptr(points), B, _ptr(out), _ptr(st))
        return out, st

    def lincomb_g1(self, scalars, points):
        """out[j] = sum_k scalars[j, k] * points[j, k]"""
        return self._lincomb("tc_g1_lincomb_batch", G1_BYTES, scalars, points)

    def lincomb_g2(self, scalars, points):
        return self._lincomb("tc_g2_lincomb_batch", G2_BYTES, scalars, points)

    def decrypt(self, t, idx, shares_g1, v, off):
        dev = self._mode(idx, shares_g1, v, off)
        self._arg(idx, (None, None), "u64", "idx")
        B, n = idx.shape
        self._arg(shares_g1, (B, n, G1_BYTES), "u8", "shares")
        self._msgs(v, off, B)
        out = self._empty(dev, tuple(v.shape), ref=v)
        st = self._empty(dev, (B,), ref=v)
        self._call("tc_decrypt_batch", int(t), int(n), _ptr(idx), _ptr(shares_g1), _ptr(v), _ptr(off), B,
                   _ptr(out), _ptr(st))
        return out, st

    def decrypt_fr(self, t, idx_fr, shares_g1, v, off):
        dev = self._mode(idx_fr, shares_g1, v, off)
        self._arg(idx_fr, (None, None, FR_BYTES), "u8", "idx_fr")
        B, n = idx_fr.shape[0], idx_fr.shape[1]
        self._arg(shares_g1, (B, n, G1_BYTES), "u8", "shares")
        self._msgs(v, off, B)
        out = self._empty(dev, tuple(v.shape), ref=v)
        st = self._empty(dev, (B,), ref=v)
        self._call("tc_decrypt_fr_batch", int(t), int(n), _ptr(idx_fr), _ptr(shares_g1), _ptr(v), _ptr(off), B, _ptr(out), _ptr(st))
        return out, st

    def decrypt_wire(self, t, idx, shares48, v, off):
        """PublicKeySet::decrypt with the decryption shares in their 48-byte compressed form (checked decode on the device)"""
        dev = self._mode(idx, shares48, v, off)
        self._arg(idx, (None, None), "u64", "idx")
        B, n = idx.shape
        self._arg(shares48, (B, n, G1_BYTES // 2), "u8", "shares48")
        self._msgs(v, off, B)
        out = self._empty(dev, tuple(v.shape), ref=v)
        st = self._empty(dev, (B,), ref=v)
        self._call("tc_decrypt_wire_batch", int(t), int(n), _ptr(idx), _ptr(shares48), _ptr(v), _ptr(off), B, _ptr(out), _ptr(st))
        return out, st

    def xor_with_hash(self, g1, data, off):
        dev = self._mode(g1, data, off)
        B = self._msgs(data, off)
        self._arg(g1, (B, G1_BYTES), "u8", "g1")
        out = self._empty(dev, tuple(data.shape), ref=data)
        st = self._empty(dev, (B,), ref=data)
        self._call("tc_xor_with_hash_batch", _ptr(g1), _ptr(data), _ptr(off), B, _ptr(out), _ptr(st))
        return out, st

    # -- pairing checks -------------------------------------------------------------------------------
    def pairing_check(self, a, b, c, d, B=None):
        """ok[j] = e(a[j], b[j]) == e(c[j], d[j]); 1-D operands are broadcast to every job."""
        dev = self._mode(a, b, c, d)
        if B is None:
            B = max(x.shape[0] if len(x.shape) == 2 else 1 for x in (a, b, c, d))
        sa, sb = self._point(a, G1_BYTES, B, "a"), self._point(b, G2_BYTES, B, "b")
        sc, sd = self._point(c, G1_BYTES, B, "c"), self._point(d, G2_BYTES, B, "d")
        ok = self._empty(dev, (B,), ref=a)
        self._call("tc_pairing_check_batch", _ptr(a), sa, _ptr(b), sb, _ptr(c), sc, _ptr(d), sd, B, _ptr(ok))
        return ok

    def verify_g2(self, pk, sig, hash_):
        dev = self._mode(pk, sig, hash_)
        self._arg(sig, (None, G2_BYTES), "u8", "sig")
        B = sig.shape[0]
        self._arg(hash_, (B, G2_BYTES), "u8", "hash")
        ok = self._empty(dev, (B,), ref=sig)
        self._call("tc_verify_g2_batch", _ptr(pk), self._point(pk, G1_BYTES, B, "pk"), _ptr(sig), _ptr(hash_), B, _ptr(ok))
        return ok

    def verify_sig(self, pk, sig, msgs, off):
        dev = self._mode(pk, sig, msgs, off)
        self._arg(sig, (None, G2_BYTES), "u8", "sig")
        B = sig.shape[0]
        self._msgs(msgs, off, B)
        ok = self._empty(dev, (B,), ref=sig)
        self._call("tc_verify_sig_batch", _ptr(pk), self._point(pk, G1_BYTES, B, "pk"), _ptr(sig), _ptr(msgs), _ptr(off), B,
                   _ptr(ok))
        return ok

    def verify_shares_rlc(self, pk_shares, sig_shares, msgs, off, seed=None):
        """Share validation by one random linear combination per message (opt-in; see tc_amd.h): returns
        (ok (B, N), number of messages that fell back to per-share checks).  `seed`: 32 secret random bytes
        (os.urandom when omitted)."""
        import os
        dev = self._mode(pk_shares, sig_shares, msgs, off)
        self._arg(pk_shares, (None, G1_BYTES), "u8", "pk_shares")
        N = pk_shares.shape[0]
        B = self._msgs(msgs, off)
        self._arg(sig_shares, (B, N, G2_BYTES), "u8", "sig_shares")
        seed = bytes(seed) if seed is not None else os.urandom(32)
        if len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        ok = self._empty(dev, (B, N), ref=sig_shares)
        nfb = ctypes.c_uint64(0)
        self._call("tc_verify_shares_rlc_batch", _ptr(pk_shares), N, _ptr(sig_shares), _ptr(msgs), _ptr(off), B, seed, _ptr(ok),
                   ctypes.byref(nfb))
        return ok, int(nfb.value)

    def verify_g2_rlc(self, pk, sig, hash_, group=0, seed=None):
        """Same-key signature batch by random linear combination (opt-in; see tc_amd.h): returns (ok (B,), number of jobs
        that fell back to per-job checks).  `seed`: 32 secret random bytes (os.urandom when omitted)."""
        import os
        dev = self._mode(pk, sig, hash_)
        self._arg(pk, (G1_BYTES,), "u8", "pk")
        self._arg(sig, (None, G2_BYTES), "u8", "sig")
        B = sig.shape[0]
        self._arg(hash_, (B, G2_BYTES), "u8", "hash")
        seed = bytes(seed) if seed is not None else os.urandom(32)
        if len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        ok = self._empty(dev, (B,), ref=sig)
        nfb = ctypes.c_uint64(0)
        self._call("tc_verify_g2_rlc_batch", _ptr(pk), _ptr(sig), _ptr(hash_), B, int(group), seed, _ptr(ok), ctypes.byref(nfb))
        return ok, int(nfb.value)

    def verify_sig_rlc(self, pk, sig, msgs, off, group=0, seed=None):
        import os
        dev = self._mode(pk, sig, msgs, off)
        self._arg(pk, (G1_BYTES,), "u8", "pk")
        self._arg(sig, (None, G2_BYTES), "u8", "sig")
        B = sig.shape[0]
        self._msgs(msgs, off, B)
        seed = bytes(seed) if seed is not None else os.urandom(32)
        if len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        ok = self._empty(dev, (B,), ref=sig)
        nfb = ctypes.c_uint64(0)
        self._call("tc_verify_sig_rlc_batch", _ptr(pk), _ptr(sig), _ptr(msgs), _ptr(off), B, int(group), seed, _ptr(ok), ctypes.byref(nfb))
        return ok, int(nfb.value)

    def _records(self, pks, key_idx, sigs, rec_off, M):
        """the operands the two ragged entries share; returns (K, R)"""
        self._arg(pks, (None, G1_BYTES), "u8", "pks")
        self._arg(sigs, (None, G2_BYTES), "u8", "sigs")
        self._arg(rec_off, (M + 1,), "u64", "rec_off")
        K, R = pks.shape[0], sigs.shape[0]
        if not _is_torch(rec_off) and int(rec_off[M]) != R:
            raise ValueError("rec_off[M] = %d, sigs holds %d records" % (int(rec_off[M]), R))
        if key_idx is not None:
            self._arg(key_idx, (R,), "u64", "key_idx")
        elif K < R:
            raise ValueError("key_idx omitted: record r uses pks[r], %d keys for %d records" % (K, R))
        return K, R

    def verify_g2_records_rlc(self, pks, key_idx, sigs, rec_off, hashes, group=0, seed=None):
        """Batch verification of ragged input (opt-in; see tc_amd.h): message m owns the records rec_off[m] .. rec_off[m + 1],
        record r is the signature sigs[r] under pks[key_idx[r]] (key_idx None: pks[r]); one Miller pair per message, one final
        exponentiation per group of `group` messages.  sigs must hold exactly rec_off[M] records.  Returns (ok (R,), number of
        records that fell back to per-record checks).  `seed`: 32 secret random bytes (os.urandom when omitted)."""
        import os
        dev = self._mode(pks, key_idx, sigs, rec_off, hashes)
        self._arg(hashes, (None, G2_BYTES), "u8", "hashes")
        M = hashes.shape[0]
        K, R = self._records(pks, key_idx, sigs, rec_off, M)
        seed = bytes(seed) if seed is not None else os.urandom(32)
        if len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        ok = self._empty(dev, (R,), ref=sigs)
        nfb = ctypes.c_uint64(0)
        self._call("tc_verify_g2_records_rlc_batch", _ptr(pks), K, _ptr(key_idx), _ptr(sigs), _ptr(rec_off), _ptr(hashes), M, int(group), seed,
                   _ptr(ok), ctypes.byref(nfb))
        return ok, int(nfb.value)

    def verify_sig_records_rlc(self, pks, key_idx, sigs, rec_off, msgs, off, group=0, seed=None):
        """verify_g2_records_rlc with the messages hashed on the device (one hash per MESSAGE)"""
        import os
        dev = self._mode(pks, key_idx, sigs, rec_off, msgs, off)
        M = self._msgs(msgs, off)
        K, R = self._records(pks, key_idx, sigs, rec_off, M)
        seed = bytes(seed) if seed is not None else os.urandom(32)
        if len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        ok = self._empty(dev, (R,), ref=sigs)
        nfb = ctypes.c_uint64(0)
        self._call("tc_verify_sig_records_rlc_batch", _ptr(pks), K, _ptr(key_idx), _ptr(sigs), _ptr(rec_off), _ptr(msgs), _ptr(off), M,
                   int(group), seed, _ptr(ok), ctypes.byref(nfb))
        return ok, int(nfb.value)

    def ciphertext_verify(self, u, v, off, w):
        dev = self._mode(u, v, off, w)
        self._arg(u, (None, G1_BYTES), "u8", "u")
        B = u.shape[0]
        self._msgs(v, off, B)
        self._arg(w, (B, G2_BYTES), "u8", "w")
        ok = self._empty(dev, (B,), ref=u)
        self._call("tc_ciphertext_verify_batch", _ptr(u), _ptr(v), _ptr(off), _ptr(w), B, _ptr(ok))
        return ok

    def ciphertext_verify_rlc(self, u, v, off, w, group=0, seed=None):
        """Ciphertext::verify for a batch by random linear combination (opt-in; see tc_amd.h): groups of `group` ciphertexts
        (0 = the default) pass with one product of pairings and ONE final exponentiation.  Returns (ok (B,), number of
        ciphertexts that fell back to per-ciphertext checks).  `seed`: 32 secret random bytes (os.urandom when omitted)."""
        import os
        dev = self._mode(u, v, off, w)
        self._arg(u, (None, G1_BYTES), "u8", "u")
        B = u.shape[0]
        self._msgs(v, off, B)
        self._arg(w, (B, G2_BYTES), "u8", "w")
        seed = bytes(seed) if seed is not None else os.urandom(32)
        if len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        ok = self._empty(dev, (B,), ref=u)
        nfb = ctypes.c_uint64(0)
        self._call("tc_ciphertext_verify_rlc_batch", _ptr(u), _ptr(v), _ptr(off), _ptr(w), B, int(group), seed, _ptr(ok), ctypes.byref(nfb))
        return ok, int(nfb.value)

    def pairing_product_check(self, a, b, n):
        """ok[j] = ( prod_{k < n} e(a[j * n + k], b[j * n + k]) == 1 ): a (B * n, 96) G1 points, b (B * n, 192) G2 points, job by
        job; an identity operand contributes the factor 1, an undecodable one gives 0."""
        n = int(n)
        if n < 1:
            raise ValueError("n: at least one pair per job")
        dev = self._mode(a, b)
        self._arg(a, (None, G1_BYTES), "u8", "a")
        if a.shape[0] % n:
            raise ValueError("a: a multiple of n points")
        self._arg(b, (a.shape[0], G2_BYTES), "u8", "b")
        B = a.shape[0] // n
        ok = self._empty(dev, (B,), ref=a)
        self._call("tc_pairing_product_check_batch", _ptr(a), _ptr(b), n, B, _ptr(ok))
        return ok

    def decrypt_share(self, fr, u, v, off, w):
        """SecretKeyShare::decrypt_share (src/lib.rs:452-457) for one key share and B ciphertexts -> (shares (B, 96), ok (B,)):
        ok[j] = Ciphertext::verify, the share of a ciphertext that fails it is the identity (the reference returns None)."""
        dev = self._mode(fr, u, v, off, w)
        self._arg(fr, (FR_BYTES,), "u8", "fr")
        self._arg(u, (None, G1_BYTES), "u8", "u")
        B = u.shape[0]
        self._msgs(v, off, B)
        self._arg(w, (B, G2_BYTES), "u8", "w")
        out = self._empty(dev, (B, G1_BYTES), ref=u)
        ok = self._empty(dev, (B,), ref=u)
        self._call("tc_decrypt_share_batch", _ptr(fr), _ptr(u), _ptr(v), _ptr(off), _ptr(w), B, _ptr(out), _ptr(ok))
        return out, ok

    def decrypt_shares(self, sk_table, idx, u, v, off, w):
        """SecretKeyShare::decrypt_share (src/lib.rs:452-457) for the n selected holders idx[j] of each of B ciphertexts, out of a
        table of N key shares -> (shares (B, n, 96), ok (B,), status (B, n)): Ciphertext::verify once per ciphertext; the shares
        of a ciphertext that fails it are identities (the reference returns None)."""
        dev = self._mode(sk_table, idx, u, v, off, w)
        self._arg(sk_table, (None, FR_BYTES), "u8", "sk_table")
        self._arg(idx, (None, None), "u64", "idx")
        B, n = idx.shape
        self._arg(u, (B, G1_BYTES), "u8", "u")
        self._msgs(v, off, B)
        self._arg(w, (B, G2_BYTES), "u8", "w")
        out = self._empty(dev, (B, n, G1_BYTES), ref=u)
        ok = self._empty(dev, (B,), ref=u)
        st = self._empty(dev, (B, n), ref=u)
        self._call("tc_decrypt_shares_batch", _ptr(sk_table), sk_table.shape[0], _ptr(idx), _ptr(u), _ptr(v), _ptr(off), _ptr(w), n, B,
                   _ptr(out), _ptr(ok), _ptr(st))
        return out, ok, st

    def secret_key_decrypt(self, fr, u, v, off, w):
        """SecretKey::decrypt (src/lib.rs:384-391) for B ciphertexts -> (plaintext bytes laid out like v, ok (B,)); the bytes
        of a ciphertext that fails Ciphertext::verify are zeros (None)."""
        dev = self._mode(fr, u, v, off, w)
        self._arg(fr, (FR_BYTES,), "u8", "fr")
        self._arg(u, (None, G1_BYTES), "u8", "u")
        B = u.shape[0]
        self._msgs(v, off, B)
        self._arg(w, (B, G2_BYTES), "u8", "w")
        out = self._empty(dev, tuple(v.shape), ref=v)
        ok = self._empty(dev, (B,), ref=u)
        self._call("tc_secret_key_decrypt_batch", _ptr(fr), _ptr(u), _ptr(v), _ptr(off), _ptr(w), B, _ptr(out), _ptr(ok))
        return out, ok

    def verify_decryption_share(self, pk_share, share, u, v, off, w):
        dev = self._mode(pk_share, share, u, v, off, w)
        self._arg(share, (None, G1_BYTES), "u8", "share")
        B = share.shape[0]
        self._arg(u, (B, G1_BYTES), "u8", "u")
        self._arg(w, (B, G2_BYTES), "u8", "w")
        self._msgs(v, off, B)
        ok = self._empty(dev, (B,), ref=share)
        self._call("tc_verify_decryption_share_batch", _ptr(pk_share), self._point(pk_share, G1_BYTES, B, "pk_share"),
                   _ptr(share), _ptr(u), _ptr(v), _ptr(off), _ptr(w), B, _ptr(ok))
        return ok

    def verify_decryption_shares_rlc(self, pk_shares, shares, u, v, off, w, seed=None):
        """Decryption-share validation by one random linear combination per ciphertext (opt-in; see tc_amd.h): returns
        (ok (B, N), number of ciphertexts that fell back to per-share checks)."""
        import os
        dev = self._mode(pk_shares, shares, u, v, off, w)
        self._arg(pk_shares, (None, G1_BYTES), "u8", "pk_shares")
        N = pk_shares.shape[0]
        self._arg(u, (None, G1_BYTES), "u8", "u")
        B = u.shape[0]
        self._arg(shares, (B, N, G1_BYTES), "u8", "shares")
        self._arg(w, (B, G2_BYTES), "u8", "w")
        self._msgs(v, off, B)
        seed = bytes(seed) if seed is not None else os.urandom(32)
        if len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        ok = self._empty(dev, (B, N), ref=shares)
        nfb = ctypes.c_uint64(0)
        self._call("tc_verify_decryption_shares_rlc_batch", _ptr(pk_shares), N, _ptr(shares), _ptr(u), _ptr(v), _ptr(off), _ptr(w), B, seed,
                   _ptr(ok), ctypes.byref(nfb))
        return ok, int(nfb.value)

    def _dshare_records(self, pks, key_idx, shares, rec_off, M):
        """the operands the two ragged decryption-share entries share; returns (K, R)"""
        self._arg(pks, (None, G1_BYTES), "u8", "pks")
        self._arg(shares, (None, G1_BYTES), "u8", "shares")
        self._arg(rec_off, (M + 1,), "u64", "rec_off")
        K, R = pks.shape[0], shares.shape[0]
        if not _is_torch(rec_off) and int(rec_off[M]) != R:
            raise ValueError("rec_off[M] = %d, shares holds %d records" % (int(rec_off[M]), R))
        if key_idx is not None:
            self._arg(key_idx, (R,), "u64", "key_idx")
        elif K < R:
            raise ValueError("key_idx omitted: record r uses pks[r], %d keys for %d records" % (K, R))
        return K, R

    def verify_decryption_share_records_rlc(self, pks, key_idx, shares, rec_off, u, v, off, w, group=0, seed=None):
        """Decryption-share validation of ragged input (opt-in; see tc_amd.h): ciphertext c owns the records rec_off[c] ..
        rec_off[c + 1], record r is the share shares[r] under pks[key_idx[r]] (key_idx None: pks[r]); two Miller pairs per
        ciphertext, one final exponentiation per group of `group` ciphertexts.  shares must hold exactly rec_off[M] records.
        Returns (ok (R,), number of records that fell back to per-record checks).  `seed`: 32 secret random bytes (os.urandom
        when omitted)."""
        import os
        dev = self._mode(pks, key_idx, shares, rec_off, u, v, off, w)
        self._arg(u, (None, G1_BYTES), "u8", "u")
        M = u.shape[0]
        self._msgs(v, off, M)
        self._arg(w, (M, G2_BYTES), "u8", "w")
        K, R = self._dshare_records(pks, key_idx, shares, rec_off, M)
        seed = bytes(seed) if seed is not None else os.urandom(32)
        if len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        ok = self._empty(dev, (R,), ref=shares)
        nfb = ctypes.c_uint64(0)
        self._call("tc_verify_decryption_share_records_rlc_batch", _ptr(pks), K, _ptr(key_idx), _ptr(shares), _ptr(rec_off), _ptr(u), _ptr(v),
                   _ptr(off), _ptr(w), M, int(group), seed, _ptr(ok), ctypes.byref(nfb))
        return ok, int(nfb.value)

    def verify_decryption_share_records_prehashed_rlc(self, pks, key_idx, shares, rec_off, hashes, w, group=0, seed=None):
        """verify_decryption_share_records_rlc with hashes[c] = hash_g1_g2(u_c, v_c) made by the caller (hash_g1_g2)"""
        import os
        dev = self._mode(pks, key_idx, shares, rec_off, hashes, w)
        self._arg(hashes, (None, G2_BYTES), "u8", "hashes")
        M = hashes.shape[0]
        self._arg(w, (M, G2_BYTES), "u8", "w")
        K, R = self._dshare_records(pks, key_idx, shares, rec_off, M)
        seed = bytes(seed) if seed is not None else os.urandom(32)
        if len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        ok = self._empty(dev, (R,), ref=shares)
        nfb = ctypes.c_uint64(0)
        self._call("tc_verify_decryption_share_records_prehashed_rlc_batch", _ptr(pks), K, _ptr(key_idx), _ptr(shares), _ptr(rec_off),
                   _ptr(hashes), _ptr(w), M, int(group), seed, _ptr(ok), ctypes.byref(nfb))
        return ok, int(nfb.value)

    # -- robust combination: validate, select and combine in one call -----------------------------------
    def combine_signatures_robust(self, commit, sig_shares, hashes=None, msgs=None, off=None, present=None, group=0, seed=None, _wire=False):
        """tc_combine_signatures_robust_batch (see tc_amd.h): commit (t+1, 96), sig_shares (B, N, 192) with slot i = node i's
        share, either hashes (B, 192) or msgs / off, present (B, N) u8 or None = all.  The first t+1 present shares of every
        message are combined and the combinations verified under the master key; only the messages whose combination does not
        verify are examined share by share.  Returns (sig (B, 192), used (B, N), bad (B, N), status (B,), number of messages
        examined share by share).  `seed`: 32 secret random bytes (os.urandom when omitted)."""
        import os
        if (hashes is None) == (off is None):
            raise ValueError("exactly one of hashes and msgs / off")
        dev = self._mode(commit, sig_shares, hashes, msgs, off, present)
        self._arg(commit, (None, G1_BYTES), "u8", "commit")
        t = commit.shape[0] - 1
        width = G2_BYTES // 2 if _wire else G2_BYTES
        self._arg(sig_shares, (None, None, width), "u8", "sig_shares")
        B, N = sig_shares.shape[0], sig_shares.shape[1]
        if t < 0 or t + 1 > N:
            raise ValueError("commit holds t+1 = %d coefficients for N = %d shares per message" % (t + 1, N))
        if hashes is not None:
            self._arg(hashes, (B, G2_BYTES), "u8", "hashes")
        else:
            self._msgs(msgs, off, B)
        if present is not None:
            self._arg(present, (B, N), "u8", "present")
        seed = bytes(seed) if seed is not None else os.urandom(32)
        if len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        out = self._empty(dev, (B, width), ref=sig_shares)
        used = self._empty(dev, (B, N), ref=sig_shares)
        bad = self._empty(dev, (B, N), ref=sig_shares)
        st = self._empty(dev, (B,), ref=sig_shares)
        nfb = ctypes.c_uint64(0)
        self._call("tc_combine_signatures_robust_wire_batch" if _wire else "tc_combine_signatures_robust_batch", _ptr(commit), t, N, _ptr(present), _ptr(sig_shares), _ptr(hashes),
                   _ptr(msgs) if off is not None else None, _ptr(off), B, int(group), seed, _ptr(out), _ptr(used), _ptr(bad), _ptr(st),
                   ctypes.byref(nfb))
        return out, used, bad, st, int(nfb.value)

    def combine_signatures_robust_wire(self, commit, sig_shares96, hashes=None, msgs=None, off=None, present=None, group=0, seed=None):
        """tc_combine_signatures_robust_wire_batch (see tc_amd.h): combine_signatures_robust on wire bytes -- sig_shares96 (B, N, 96)
        holds SignatureShare::to_bytes forms, always through the checked decode -- of which only the t+1 selected shares of a
        message are decoded; membership is tested on the combination.  Returns (sig (B, 96) = Signature::to_bytes, the identity's
        0xC0 form for a message that did not end OK, used, bad, status, number of messages examined share by share)."""
        return self.combine_signatures_robust(commit, sig_shares96, hashes=hashes, msgs=msgs, off=off, present=present, group=group, seed=seed,
                                              _wire=True)

    def decrypt_robust_wire(self, commit, shares48, u, v, off, w, present=None):
        """tc_decrypt_robust_wire_batch (see tc_amd.h): decrypt_robust on wire bytes, shares48 (B, N, 48) compressed decryption
        shares; everything else, and the result, as decrypt_robust."""
        return self.decrypt_robust(commit, shares48, u, v, off, w, present=present, _wire=True)

    def decrypt_robust(self, commit, shares, u, v, off, w, present=None, _wire=False):
        """tc_decrypt_robust_batch (see tc_amd.h): commit (t+1, 96), shares (B, N, 96) with slot i = node i's decryption share
        of ciphertext (u, v, w)[j], present (B, N) u8 or None = all.  Returns (plaintext bytes laid out like v -- zeros for a
        ciphertext that did not end OK --, used (B, N), bad (B, N), status (B,), number of ciphertexts examined share by
        share)."""
        dev = self._mode(commit, shares, u, v, off, w, present)
        self._arg(commit, (None, G1_BYTES), "u8", "commit")
        t = commit.shape[0] - 1
        self._arg(shares, (None, None, G1_BYTES // 2 if _wire else G1_BYTES), "u8", "shares")
        B, N = shares.shape[0], shares.shape[1]
        if t < 0 or t + 1 > N:
            raise ValueError("commit holds t+1 = %d coefficients for N = %d shares per ciphertext" % (t + 1, N))
        self._arg(u, (B, G1_BYTES), "u8", "u")
        self._arg(w, (B, G2_BYTES), "u8", "w")
        self._msgs(v, off, B)
        if present is not None:
            self._arg(present, (B, N), "u8", "present")
        out = self._empty(dev, tuple(v.shape), ref=v)
        used = self._empty(dev, (B, N), ref=shares)
        bad = self._empty(dev, (B, N), ref=shares)
        st = self._empty(dev, (B,), ref=shares)
        nfb = ctypes.c_uint64(0)
        self._call("tc_decrypt_robust_wire_batch" if _wire else "tc_decrypt_robust_batch", _ptr(commit), t, N, _ptr(present), _ptr(shares), _ptr(u), _ptr(v), _ptr(off), _ptr(w), B,
                   _ptr(out), _ptr(used), _ptr(bad), _ptr(st), ctypes.byref(nfb))
        return out, used, bad, st, int(nfb.value)

    # -- membership tests -----------------------------------------------------------------------------
    def g1_subgroup_check(self, pts):
        """ok[j] = pts[j] is a valid encoding of a point of G1 (on the curve, order r)"""
        dev = self._mode(pts)
        self._arg(pts, (None, G1_BYTES), "u8", "pts")
        ok = self._empty(dev, (pts.shape[0],), ref=pts)
        self._call("tc_g1_subgroup_check_batch", _ptr(pts), pts.shape[0], _ptr(ok))
        return ok

    def g2_subgroup_check(self, pts):
        dev = self._mode(pts)
        self._arg(pts, (None, G2_BYTES), "u8", "pts")
        ok = self._empty(dev, (pts.shape[0],), ref=pts)
        self._call("tc_g2_subgroup_check_batch", _ptr(pts), pts.shape[0], _ptr(ok))
        return ok

    # -- wire formats ------------------------------------------------------------------------------------
    def _recode(self, name, a, nin, nout):
        dev = self._mode(a)
        self._arg(a, (None, nin), "u8", "points")
        B = a.shape[0]
        out = self._empty(dev, (B, nout), ref=a)
        st = self._empty(dev, (B,), ref=a)
        self._call(name, _ptr(a), B, _ptr(out), _ptr(st))
        return out, st

    def g1_compress(self, pts):
        return self._recode("tc_g1_compress_batch", pts, G1_BYTES, 48)

    def g2_compress(self, pts):
        return self._recode("tc_g2_compress_batch", pts, G2_BYTES, 96)

    def g1_decompress(self, comp):
        """checked decode of 48-byte compressed G1 (from_bytes): status 3 = invalid"""
        return self._recode("tc_g1_decompress_batch", comp, 48, G1_BYTES)

    def g2_decompress(self, comp):
        return self._recode("tc_g2_decompress_batch", comp, 96, G2_BYTES)

    def encrypt(self, pk, r, msgs, off):
        """PublicKey::encrypt_with_rng with the Fr draws supplied: returns (u, v, w, status)."""
        dev = self._mode(pk, r, msgs, off)
        B = self._msgs(msgs, off)
        self._arg(r, (B, FR_BYTES), "u8", "r")
        u = self._empty(dev, (B, G1_BYTES), ref=r)
        v = self._empty(dev, tuple(msgs.shape), ref=r)
        w = self._empty(dev, (B, G2_BYTES), ref=r)
        st = self._empty(dev, (B,), ref=r)
        self._call("tc_encrypt_batch", _ptr(pk), self._point(pk, G1_BYTES, B, "pk"), _ptr(r), _ptr(msgs), _ptr(off), B, _ptr(u),
                   _ptr(v), _ptr(w), _ptr(st))
        return u, v, w, st

    def public_key_shares(self, commit, idx):
        """Commitment::evaluate(idx + 1) for every index: (M, 96)."""
        dev = self._mode(commit, idx)
        self._arg(commit, (None, G1_BYTES), "u8", "commit")
        self._arg(idx, (None,), "u64", "idx")
        M = idx.shape[0]
        t = commit.shape[0] - 1
        out = self._empty(dev, (M, G1_BYTES), ref=commit)
        st = self._empty(dev, (M,), ref=commit)
        self._call("tc_public_key_share_batch", _ptr(commit), int(t), _ptr(idx), M, _ptr(out), _ptr(st))
        return out, st

    # -- DKG algebra (src/poly.rs) ------------------------------------------------------------------------
    def g1_commitment(self, coeff_fr):
        """out[i] = coeff_fr[i] * g1 (Poly::commitment / BivarPoly::commitment): fixed-base, LDS window table"""
        dev = self._mode(coeff_fr)
        self._arg(coeff_fr, (None, FR_BYTES), "u8", "coeff_fr")
        M = coeff_fr.shape[0]
        out = self._empty(dev, (M, G1_BYTES), ref=coeff_fr)
        st = self._empty(dev, (M,), ref=coeff_fr)
        self._call("tc_g1_commitment_batch", _ptr(coeff_fr), M, _ptr(out), _ptr(st))
        return out, st

    def bivar_commitment_rows(self, commit, degree, xs):
        """BivarCommitment::row(xs[m]) for every m: (M, degree+1, 96)"""
        dev = self._mode(commit, xs)
        n = (degree + 1) * (degree + 2) // 2
        self._arg(commit, (n, G1_BYTES), "u8", "commit")
        self._arg(xs, (None,), "u64", "xs")
        M = xs.shape[0]
        out = self._empty(dev, (M, degree + 1, G1_BYTES), ref=commit)
        st = self._empty(dev, (M, degree + 1), ref=commit)
        self._call("tc_bivar_commitment_row_batch", _ptr(commit), int(degree), _ptr(xs), M, _ptr(out), _ptr(st))
        return out, st

    def fr_interpolate(self, xs, ys):
        """Poly::interpolate for B jobs of n samples: xs, ys (B, n, 32) -> coefficients (B, n, 32), status (B,)"""
        dev = self._mode(xs, ys)
        self._arg(xs, (None, None, FR_BYTES), "u8", "xs")
        B, n = xs.shape[0], xs.shape[1]
        self._arg(ys, (B, n, FR_BYTES), "u8", "ys")
        out = self._empty(dev, (B, n, FR_BYTES), ref=xs)
        st = self._empty(dev, (B,), ref=xs)
        self._call("tc_fr_interpolate_batch", int(n), _ptr(xs), _ptr(ys), B, _ptr(out), _ptr(st))
        return out, st

    # -- DKG verification: the secret side and the two checks (src/poly.rs:838-878) ---------------------------
    def fr_poly_evaluate(self, coeff_fr, xs_fr):
        """Poly::evaluate for B polynomials of n coefficients at M shared abscissae: coeff_fr (B, n, 32), xs_fr (M, 32) ->
        values (B, M, 32), status (B, M)"""
        dev = self._mode(coeff_fr, xs_fr)
        self._arg(coeff_fr, (None, None, FR_BYTES), "u8", "coeff_fr")
        B, n = coeff_fr.shape[0], coeff_fr.shape[1]
        self._arg(xs_fr, (None, FR_BYTES), "u8", "xs_fr")
        M = xs_fr.shape[0]
        out = self._empty(dev, (B, M, FR_BYTES), ref=xs_fr)
        st = self._empty(dev, (B, M), ref=xs_fr)
        self._call("tc_fr_poly_evaluate_batch", _ptr(coeff_fr) if n else None, int(n), _ptr(xs_fr), M, B, _ptr(out), _ptr(st))
        return out, st

    def bivar_poly_rows(self, coeff_fr, degree, xs):
        """BivarPoly::row(xs[m]) for every m: coeff_fr ((degree+1)(degree+2)/2, 32) -> rows (M, degree+1, 32), status (M, degree+1)"""
        dev = self._mode(coeff_fr, xs)
        self._arg(coeff_fr, ((degree + 1) * (degree + 2) // 2, FR_BYTES), "u8", "coeff_fr")
        self._arg(xs, (None,), "u64", "xs")
        M = xs.shape[0]
        out = self._empty(dev, (M, degree + 1, FR_BYTES), ref=coeff_fr)
        st = self._empty(dev, (M, degree + 1), ref=coeff_fr)
        self._call("tc_bivar_poly_row_batch", _ptr(coeff_fr), int(degree), _ptr(xs), M, _ptr(out), _ptr(st))
        return out, st

    def dkg_verify_rows(self, commits, degree, xs, row_fr):
        """`row_poly.commitment() == bi_commit.row(m)` for B parts: commits (B, ncoeff, 96), or (ncoeff, 96) for ONE commitment
        shared by every job; xs (B,); row_fr (B, degree+1, 32) -> the row commitments (B, degree+1, 96), ok (B,)"""
        dev = self._mode(commits, xs, row_fr)
        ncoeff = (degree + 1) * (degree + 2) // 2
        self._arg(xs, (None,), "u64", "xs")
        B = xs.shape[0]
        if len(commits.shape) == 2:
            self._arg(commits, (ncoeff, G1_BYTES), "u8", "commits")
            stride = 0
        else:
            self._arg(commits, (B, ncoeff, G1_BYTES), "u8", "commits")
            stride = ncoeff * G1_BYTES
        self._arg(row_fr, (B, degree + 1, FR_BYTES), "u8", "row_fr")
        rows = self._empty(dev, (B, degree + 1, G1_BYTES), ref=commits)
        ok = self._empty(dev, (B,), ref=commits)
        self._call("tc_dkg_verify_rows_batch", _ptr(commits), stride, int(degree), _ptr(xs), _ptr(row_fr), B, _ptr(rows), _ptr(ok))
        return rows, ok

    def _dkg_values(self, rows, xs, vals_fr):
        self._arg(rows, (None, None, G1_BYTES), "u8", "rows")
        B, degree = rows.shape[0], rows.shape[1] - 1
        if degree < 0:
            raise ValueError("rows: a row commitment holds at least one point")
        self._arg(xs, (B, None), "u64", "xs")
        n = xs.shape[1]
        self._arg(vals_fr, (B, n, FR_BYTES), "u8", "vals_fr")
        return B, degree, n

    def dkg_verify_values(self, rows, xs, vals_fr):
        """`bi_commit.evaluate(m, s) == g1 * val` for B parts of n values: rows (B, degree+1, 96), xs (B, n), vals_fr (B, n, 32)
        -> ok (B, n)"""
        dev = self._mode(rows, xs, vals_fr)
        B, degree, n = self._dkg_values(rows, xs, vals_fr)
        ok = self._empty(dev, (B, n), ref=rows)
        self._call("tc_dkg_verify_values_batch", _ptr(rows), int(degree), _ptr(xs), _ptr(vals_fr), n, B, _ptr(ok))
        return ok

    def dkg_verify_values_rlc(self, rows, xs, vals_fr, seed=None):
        """The same ok (B, n) by one random linear combination per part (opt-in; see tc_amd.h): returns (ok, number of parts
        that fell back to the value-by-value checks).  `seed`: 32 secret random bytes (os.urandom when omitted)."""
        import os
        dev = self._mode(rows, xs, vals_fr)
        B, degree, n = self._dkg_values(rows, xs, vals_fr)
        seed = bytes(seed) if seed is not None else os.urandom(32)
        if len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        ok = self._empty(dev, (B, n), ref=rows)
        nfb = ctypes.c_uint64(0)
        self._call("tc_dkg_verify_values_rlc_batch", _ptr(rows), int(degree), _ptr(xs), _ptr(vals_fr), n, B, seed, _ptr(ok),
                   ctypes.byref(nfb))
        return ok, int(nfb.value)

    # -- DKG finalisation: the accepted parts summed into the key set (src/poly.rs:870-876, 895-898) ----------
    def _mask(self, mask, n, name):
        if mask is not None:
            self._arg(mask, (n,), "u8", name)
        return _ptr(mask) if mask is not None else None

    def g1_sum(self, pts, mask=None):
        """Commitment::add_assign folded over n terms: pts (n, B, 96) -> out[j] = sum of the included pts[k, j]: (B, 96),
        status (B,).  mask (n,) u8 (0 = excluded, never decoded) or None = all."""
        dev = self._mode(pts, mask)
        self._arg(pts, (None, None, G1_BYTES), "u8", "pts")
        n, B = pts.shape[0], pts.shape[1]
        return self._g1_sum(dev, pts, B * G1_BYTES, n, mask, B)

    def g1_sum_strided(self, pts, B, mask=None):
        """g1_sum over the first B of the S >= B points of every term: pts (n, S, 96), term stride S * 96 bytes"""
        dev = self._mode(pts, mask)
        self._arg(pts, (None, None, G1_BYTES), "u8", "pts")
        n, S = pts.shape[0], pts.shape[1]
        if not 0 <= int(B) <= S:
            raise ValueError("B: at most the %d points a term holds" % S)
        return self._g1_sum(dev, pts, S * G1_BYTES, n, mask, int(B))

    def _g1_sum(self, dev, pts, stride, n, mask, B):
        out = self._empty(dev, (B, G1_BYTES), ref=pts)
        st = self._empty(dev, (B,), ref=pts)
        self._call("tc_g1_sum_batch", _ptr(pts) if n else None, stride, n, self._mask(mask, n, "mask"), B, _ptr(out), _ptr(st))
        return out, st

    def bivar_row0_sum(self, commits, degree, mask=None):
        """`sum_commit += bi_commit.row(0)` over the included parts: commits (P, S, 96) with S >= (degree+1)(degree+2)/2 points per
        part -> (degree+1, 96), status (degree+1,)"""
        dev = self._mode(commits, mask)
        self._arg(commits, (None, None, G1_BYTES), "u8", "commits")
        P, S = commits.shape[0], commits.shape[1]
        if S < (degree + 1) * (degree + 2) // 2:
            raise ValueError("commits: a commitment of degree %d holds %d points" % (degree, (degree + 1) * (degree + 2) // 2))
        out = self._empty(dev, (degree + 1, G1_BYTES), ref=commits)
        st = self._empty(dev, (degree + 1,), ref=commits)
        if P == 0:                                   # the empty sum (the C entry treats P = 0 as a no-op)
            out[:] = 0
            out[:, 0] = 0x40
            st[:] = 0
            return out, st
        self._call("tc_bivar_commitment_row0_sum_batch", _ptr(commits), S * G1_BYTES, int(degree), P, self._mask(mask, P, "mask"), _ptr(out),
                   _ptr(st))
        return out, st

    def fr_sum(self, vals_fr, mask=None):
        """Poly::add_assign per coefficient: vals_fr (n, B, 32) -> out[j] = sum of the included vals_fr[k, j] mod r: (B, 32), status (B,)"""
        dev = self._mode(vals_fr, mask)
        self._arg(vals_fr, (None, None, FR_BYTES), "u8", "vals_fr")
        n, B = vals_fr.shape[0], vals_fr.shape[1]
        out = self._empty(dev, (B, FR_BYTES), ref=vals_fr)
        st = self._empty(dev, (B,), ref=vals_fr)
        self._call("tc_fr_sum_batch", _ptr(vals_fr) if n else None, B * FR_BYTES, n, self._mask(mask, n, "mask"), B, _ptr(out), _ptr(st))
        return out, st

    def dkg_generate(self, commits, degree, accept=None, xs=None, vals_fr=None):
        """The finalisation in one call: commits (P, S, 96), accept (P,) u8 or None = all, and for a node with a secret its samples
        xs (P, n_v) u64 and vals_fr (P, n_v, 32) -> (the key set's commitment (degree+1, 96), the share (32,) or None, part_status
        (P,)).  When an accepted part fails, the commitment is identities and the share zero."""
        dev = self._mode(commits, accept, xs, vals_fr)
        self._arg(commits, (None, None, G1_BYTES), "u8", "commits")
        P, S = commits.shape[0], commits.shape[1]
        if S < (degree + 1) * (degree + 2) // 2:
            raise ValueError("commits: a commitment of degree %d holds %d points" % (degree, (degree + 1) * (degree + 2) // 2))
        if (xs is None) != (vals_fr is None):
            raise ValueError("xs and vals_fr come together")
        n_v = 0
        if xs is not None:
            self._arg(xs, (P, None), "u64", "xs")
            n_v = xs.shape[1]
            self._arg(vals_fr, (P, n_v, FR_BYTES), "u8", "vals_fr")
        out = self._empty(dev, (degree + 1, G1_BYTES), ref=commits)
        share = self._empty(dev, (FR_BYTES,), ref=commits) if xs is not None else None
        st = self._empty(dev, (P,), ref=commits)
        if P == 0:
            out[:] = 0
            out[:, 0] = 0x40
            if share is not None:
                share[:] = 0
            return out, share, st
        self._call("tc_dkg_generate_batch", _ptr(commits), S * G1_BYTES, int(degree), P, self._mask(accept, P, "accept"),
                   _ptr(xs) if n_v else None, _ptr(vals_fr) if n_v else None, n_v, _ptr(out), _ptr(share) if share is not None else None, _ptr(st))
        return out, share, st

    # -- DKG resharing: the same sums with Lagrange weights (src/poly.rs:210-254, 462-471; src/lib.rs:719-767) ----------
    def g1_weighted_sum(self, pts, weights_fr, mask=None):
        """pts (n, B, 96), weights_fr (n, 32) canonical LE, public -> out[j] = sum of the included weights[k] * pts[k, j]: (B, 96),
        status (B,).  An included term with a non-canonical weight fails every output."""
        dev = self._mode(pts, weights_fr, mask)
        self._arg(pts, (None, None, G1_BYTES), "u8", "pts")
        n, B = pts.shape[0], pts.shape[1]
        self._arg(weights_fr, (n, FR_BYTES), "u8", "weights_fr")
        out = self._empty(dev, (B, G1_BYTES), ref=pts)
        st = self._empty(dev, (B,), ref=pts)
        self._call("tc_g1_weighted_sum_batch", _ptr(pts) if n else None, B * G1_BYTES, n, _ptr(weights_fr) if n else None, self._mask(mask, n, "mask"),
                   B, _ptr(out), _ptr(st))
        return out, st

    def fr_weighted_sum(self, vals_fr, weights_fr, mask=None):
        """vals_fr (n, B, 32) secret, weights_fr (n, 32) public -> out[j] = sum of the included weights[k] * vals_fr[k, j] mod r:
        (B, 32), status (B,)"""
        dev = self._mode(vals_fr, weights_fr, mask)
        self._arg(vals_fr, (None, None, FR_BYTES), "u8", "vals_fr")
        n, B = vals_fr.shape[0], vals_fr.shape[1]
        self._arg(weights_fr, (n, FR_BYTES), "u8", "weights_fr")
        out = self._empty(dev, (B, FR_BYTES), ref=vals_fr)
        st = self._empty(dev, (B,), ref=vals_fr)
        self._call("tc_fr_weighted_sum_batch", _ptr(vals_fr) if n else None, B * FR_BYTES, n, _ptr(weights_fr) if n else None,
                   self._mask(mask, n, "mask"), B, _ptr(out), _ptr(st))
        return out, st

    def dkg_reshare(self, old_commit, dealer_idx, commits, degree, accept=None, xs=None, vals_fr=None):
        """The finalisation of a resharing: old_commit (t_old+1, 96), dealer_idx (P,) u64 (part p is dealt by old node dealer_idx[p]),
        commits / accept / xs / vals_fr as in dkg_generate -> (the new commitment (degree+1, 96), the share (32,) or None, used (P,),
        part_status (P,), status (1,)).  Unless status is 0 the commitment is identities, the share zero and used all zero."""
        dev = self._mode(old_commit, dealer_idx, commits, accept, xs, vals_fr)
        self._arg(old_commit, (None, G1_BYTES), "u8", "old_commit")
        self._arg(commits, (None, None, G1_BYTES), "u8", "commits")
        P, S = commits.shape[0], commits.shape[1]
        self._arg(dealer_idx, (P,), "u64", "dealer_idx")
        if old_commit.shape[0] < 1:
            raise ValueError("old_commit: at least one coefficient")
        if S < (degree + 1) * (degree + 2) // 2:
            raise ValueError("commits: a commitment of degree %d holds %d points" % (degree, (degree + 1) * (degree + 2) // 2))
        if (xs is None) != (vals_fr is None):
            raise ValueError("xs and vals_fr come together")
        n_v = 0
        if xs is not None:
            self._arg(xs, (P, None), "u64", "xs")
            n_v = xs.shape[1]
            self._arg(vals_fr, (P, n_v, FR_BYTES), "u8", "vals_fr")
        out = self._empty(dev, (degree + 1, G1_BYTES), ref=commits)
        share = self._empty(dev, (FR_BYTES,), ref=commits) if xs is not None else None
        used = self._empty(dev, (P,), ref=commits)
        st = self._empty(dev, (P,), ref=commits)
        status = self._empty(dev, (1,), ref=commits)
        if P == 0:                                   # nobody dealt (the C entry treats P = 0 as a no-op)
            out[:] = 0
            out[:, 0] = 0x40
            if share is not None:
                share[:] = 0
            status[:] = _native.JOB_NOT_ENOUGH_SHARES
            return out, share, used, st, status
        self._call("tc_dkg_reshare_batch", _ptr(old_commit), old_commit.shape[0] - 1, _ptr(dealer_idx), _ptr(commits), S * G1_BYTES, int(degree), P,
                   self._mask(accept, P, "accept"), _ptr(xs) if n_v else None, _ptr(vals_fr) if n_v else None, n_v, _ptr(out),
                   _ptr(share) if share is not None else None, _ptr(used), _ptr(st), _ptr(status))
        return out, share, used, st, status


class Group:
    """tc_group: several GPUs of one node driven from this process (one worker thread per GPU inside the library),
    host-memory batches sharded contiguously, key-set broadcast and valid-count all-reduce on RCCL."""

    def __init__(self, devices):
        self._lib = _native.load()
        g = ctypes.c_void_p()
        arr = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        rc = self._lib.tc_group_create(ctypes.byref(g), arr, len(devices))
        if rc != _native.TC_OK:
            raise TcError(rc, "tc_group_create failed for devices %s" % (list(devices),))
        self._g = g
        self.t = None

    def close(self):
        if getattr(self, "_g", None):
            self._lib.tc_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, *args):
        rc = getattr(self._lib, name)(self._g, *args)
        if rc != _native.TC_OK:
            raise TcError(rc, self._lib.tc_group_last_error(self._g).decode())

    def size(self):
        return int(self._lib.tc_group_size(self._g))

    def uses_rccl(self):
        return bool(self._lib.tc_group_uses_rccl(self._g))

    def shard(self, B, rank):
        s, c = ctypes.c_size_t(), ctypes.c_size_t()
        self._call("tc_group_shard", int(B), int(rank), ctypes.byref(s), ctypes.byref(c))
        return int(s.value), int(c.value)

    def set_keyset(self, commit):
        Engine._arg(commit, (None, G1_BYTES), "u8", "commit")
        self._call("tc_group_set_keyset", commit.shape[0] - 1, _ptr(commit))
        self.t = commit.shape[0] - 1

    def get_keyset(self, rank):
        out = np.empty((self.t + 1, G1_BYTES), dtype=np.uint8)
        self._call("tc_group_get_keyset", int(rank), _ptr(out))
        return out

    def combine_signatures(self, idx, shares):
        Engine._arg(idx, (None, None), "u64", "idx")
        B, n = idx.shape
        Engine._arg(shares, (B, n, G2_BYTES), "u8", "shares")
        out = np.empty((B, G2_BYTES), dtype=np.uint8)
        st = np.empty(B, dtype=np.uint8)
        self._call("tc_group_combine_signatures", n, _ptr(idx), _ptr(shares), B, _ptr(out), _ptr(st))
        return out, st

    def verify_g2(self, sig, hashes):
        Engine._arg(sig, (None, G2_BYTES), "u8", "sig")
        B = sig.shape[0]
        Engine._arg(hashes, (B, G2_BYTES), "u8", "hashes")
        ok = np.empty(B, dtype=np.uint8)
        nv = ctypes.c_uint64(0)
        self._call("tc_group_verify_g2", _ptr(sig), _ptr(hashes), B, _ptr(ok), ctypes.byref(nv))
        return ok, int(nv.value)

    def transfer_bytes(self):
        """(host-to-device, device-to-host) bytes the group and its contexts have moved over PCIe"""
        up, down = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._call("tc_group_transfer_bytes", ctypes.byref(up), ctypes.byref(down))
        return int(up.value), int(down.value)

    def sign_combine_verify(self, sk_table, idx, msgs, off):
        Engine._arg(sk_table, (None, FR_BYTES), "u8", "sk_table")
        Engine._arg(idx, (None, None), "u64", "idx")
        B, n = idx.shape
        # the same operand validation as the single-GPU Engine: dtype, contiguity, B + 1 offsets
        Engine._arg(off, (B + 1,), "u64", "off")
        Engine._arg(msgs, (None,), "u8", "msgs")
        if int(off[0]) != 0 or (np.diff(off.astype(np.int64)) < 0).any() or int(off[-1]) > msgs.shape[0]:
            raise ValueError("off must start at 0, be non-decreasing and end inside msgs")
        sig = np.empty((B, G2_BYTES), dtype=np.uint8)
        ok = np.empty(B, dtype=np.uint8)
        nv = ctypes.c_uint64(0)
        self._call("tc_group_sign_combine_verify", _ptr(sk_table), sk_table.shape[0], _ptr(idx), n, _ptr(msgs), _ptr(off), B, _ptr(sig),
                   _ptr(ok), ctypes.byref(nv))
        return sig, ok, int(nv.value)
