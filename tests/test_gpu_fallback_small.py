"""The combined entries and their fallbacks at the smallest shapes that reach every branch of the host code that drives them
(tc_api.hip: Call::upload / readback / require_members / take_verdicts, Compacted; tc_fallback.h): per entry the verdicts, n_fallback
and the bytes the call moved over PCIe (tc_ctx_transfer_bytes), with input checks on and off, clean and with one planted fault.

  * per message / per ciphertext (verify_shares_rlc, verify_decryption_shares_rlc) and the four robust combiners, each share by
    share and by bisection: t = 1, N = 3, B = 3, the bad share in the last job (robust: among its first t + 1 present shares, so
    pass 1 fails and pass 2 runs);
  * grouped (verify_g2_rlc, verify_sig_rlc, ciphertext_verify_rlc): B = 5, group = 2 -- two full groups and a tail of one; the
    fault in job 4 (only the tail falls back), in job 0, then everywhere (a wrong key; a ciphertext names no key: one fault in
    every group instead);
  * records: M = 3 messages of 2, 0 and 1 records, K = 2 keys through key_idx, group = 2; the bad record in the last message,
    in the first, and (checked mode) a key table entry outside G1 that only message 0 names; the same for the decryption shares
    of M = 3 ciphertexts (verify_decryption_share_records_rlc and its pre-hashed form); and that last case once more per entry
    with every operand in device memory -- the only path through the read-back of key_idx, which the host needs only when a key
    table entry is bad;
  * DKG values: degree 1, n = 2, B = 3, one wrong value in job 2.

The expected verdicts come from the matching per-item entry on the same (expanded) arrays, one item per case also from the
oracle; the robust expectations from the model of tests/test_gpu_robust.py; n_fallback from the model of
tests/test_gpu_pairing_product.py (_fallback; per message: group = 1).  The transfer bytes are what the entries moved before the
staging helpers existed: TRANSFERS below was printed by this file, its assertion replaced by the print, on commit 5eb9372.  The
pairs of the decryption records and of the device-I/O cases (the last block of TRANSFERS) were printed the same way on commit
735d348, the parent of the change that folded the bad-group rule and the front end of the two records entries into one copy."""
import random

import numpy as np
import pytest

import c_oracle as c
import tc_oracle as o
from threshold_crypto_amd.engine import pack_messages
from test_gpu_pairing_product import _fallback
from test_gpu_robust import EncWorld, IDENT2, OK, Plan, SigWorld, as_lists, fr_rows, non_member_g1, u8

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
KEY = bytes(range(64, 96))
T, N, B3, B5, GROUP = 1, 3, 3, 5, 2

# (h2d, d2h) bytes of one call, host I/O; recorded on commit 5eb9372 (the parent of the change that introduced the helpers)
TRANSFERS = {
    'verify_shares_rlc checked clean': (2128, 15),
    'verify_shares_rlc checked bad': (2164, 15),
    'verify_shares_rlc unchecked clean': (2128, 15),
    'verify_shares_rlc unchecked bad': (2164, 15),
    'verify_g2_rlc checked clean': (2048, 25),
    'verify_g2_rlc checked bad4': (2052, 25),
    'verify_g2_rlc checked bad0': (2056, 25),
    'verify_g2_rlc checked wrong_key': (2068, 25),
    'verify_sig_rlc checked clean': (1216, 20),
    'verify_sig_rlc checked bad4': (1220, 20),
    'verify_sig_rlc checked bad0': (1224, 20),
    'verify_sig_rlc checked wrong_key': (1236, 20),
    'verify_g2_rlc unchecked clean': (2048, 14),
    'verify_g2_rlc unchecked bad4': (2052, 14),
    'verify_g2_rlc unchecked bad0': (2056, 14),
    'verify_g2_rlc unchecked wrong_key': (2068, 14),
    'verify_sig_rlc unchecked clean': (1216, 14),
    'verify_sig_rlc unchecked bad4': (1220, 14),
    'verify_sig_rlc unchecked bad0': (1224, 14),
    'verify_sig_rlc unchecked wrong_key': (1236, 14),
    'ciphertext_verify_rlc checked clean': (1555, 31),
    'ciphertext_verify_rlc checked bad4': (1559, 31),
    'ciphertext_verify_rlc checked bad0': (1563, 31),
    'ciphertext_verify_rlc checked every_group': (1575, 31),
    'ciphertext_verify_rlc unchecked clean': (1555, 21),
    'ciphertext_verify_rlc unchecked bad4': (1559, 21),
    'ciphertext_verify_rlc unchecked bad0': (1563, 21),
    'ciphertext_verify_rlc unchecked every_group': (1575, 21),
    'verify_g2_records_rlc checked clean': (1848, 20),
    'verify_g2_records_rlc checked bad_last': (1856, 20),
    'verify_g2_records_rlc checked bad_first': (1864, 20),
    'verify_g2_records_rlc checked key_outside_g1': (1864, 20),
    'verify_sig_records_rlc checked clean': (1352, 17),
    'verify_sig_records_rlc checked bad_last': (1360, 17),
    'verify_sig_records_rlc checked bad_first': (1368, 17),
    'verify_sig_records_rlc checked key_outside_g1': (1368, 17),
    'verify_g2_records_rlc unchecked clean': (1848, 12),
    'verify_g2_records_rlc unchecked bad_last': (1856, 12),
    'verify_g2_records_rlc unchecked bad_first': (1864, 12),
    'verify_sig_records_rlc unchecked clean': (1352, 12),
    'verify_sig_records_rlc unchecked bad_last': (1360, 12),
    'verify_sig_records_rlc unchecked bad_first': (1368, 12),
    'verify_decryption_shares_rlc checked clean': (2114, 21),
    'verify_decryption_shares_rlc checked bad': (2150, 21),
    'verify_decryption_shares_rlc unchecked clean': (2114, 21),
    'verify_decryption_shares_rlc unchecked bad': (2150, 21),
    'dkg_verify_values_rlc checked clean': (848, 9),
    'dkg_verify_values_rlc checked bad': (860, 9),
    'dkg_verify_values_rlc unchecked clean': (848, 9),
    'dkg_verify_values_rlc unchecked bad': (860, 9),
    'robust_sig per_share checked clean': (2561, 608),
    'robust_sig per_share checked bad': (2613, 608),
    'robust_sig bisect checked clean': (2561, 608),
    'robust_sig bisect checked bad': (2712, 618),
    'robust_sig_wire per_share checked clean': (1697, 320),
    'robust_sig_wire per_share checked bad': (1749, 320),
    'robust_sig_wire bisect checked clean': (1697, 320),
    'robust_sig_wire bisect checked bad': (1848, 330),
    'robust_dec per_share checked clean': (2019, 63),
    'robust_dec per_share checked bad': (2059, 63),
    'robust_dec bisect checked clean': (2019, 63),
    'robust_dec bisect checked bad': (2158, 73),
    'robust_dec_wire per_share checked clean': (1587, 63),
    'robust_dec_wire per_share checked bad': (1627, 63),
    'robust_dec_wire bisect checked clean': (1587, 63),
    'robust_dec_wire bisect checked bad': (1726, 73),
    'robust_sig per_share unchecked clean': (2561, 606),
    'robust_sig per_share unchecked bad': (2613, 606),
    'robust_sig bisect unchecked clean': (2561, 606),
    'robust_sig bisect unchecked bad': (2712, 616),
    'robust_sig_wire per_share unchecked clean': (1697, 318),
    'robust_sig_wire per_share unchecked bad': (1749, 318),
    'robust_sig_wire bisect unchecked clean': (1697, 318),
    'robust_sig_wire bisect unchecked bad': (1848, 328),
    'robust_dec per_share unchecked clean': (2019, 61),
    'robust_dec per_share unchecked bad': (2059, 61),
    'robust_dec bisect unchecked clean': (2019, 61),
    'robust_dec bisect unchecked bad': (2158, 71),
    'robust_dec_wire per_share unchecked clean': (1587, 61),
    'robust_dec_wire per_share unchecked bad': (1627, 61),
    'robust_dec_wire bisect unchecked clean': (1587, 61),
    'robust_dec_wire bisect unchecked bad': (1726, 71),
    # recorded on commit 735d348 (the device_io cases: every operand in device memory)
    'verify_g2_records_rlc checked key_outside_g1 device_io': (496, 73),
    'verify_sig_records_rlc checked key_outside_g1 device_io': (496, 78),
    'verify_decryption_share_records_rlc checked clean': (2106, 22),
    'verify_decryption_share_records_rlc checked bad_last': (2114, 22),
    'verify_decryption_share_records_rlc checked bad_first': (2122, 22),
    'verify_decryption_share_records_rlc checked key_outside_g1': (2122, 22),
    'verify_decryption_share_records_prehashed_rlc checked clean': (2328, 22),
    'verify_decryption_share_records_prehashed_rlc checked bad_last': (2336, 22),
    'verify_decryption_share_records_prehashed_rlc checked bad_first': (2344, 22),
    'verify_decryption_share_records_prehashed_rlc checked key_outside_g1': (2344, 22),
    'verify_decryption_share_records_rlc unchecked clean': (2106, 11),
    'verify_decryption_share_records_rlc unchecked bad_last': (2114, 11),
    'verify_decryption_share_records_rlc unchecked bad_first': (2122, 11),
    'verify_decryption_share_records_prehashed_rlc unchecked clean': (2328, 11),
    'verify_decryption_share_records_prehashed_rlc unchecked bad_last': (2336, 11),
    'verify_decryption_share_records_prehashed_rlc unchecked bad_first': (2344, 11),
    'verify_decryption_share_records_rlc checked key_outside_g1 device_io': (688, 83),
    'verify_decryption_share_records_prehashed_rlc checked key_outside_g1 device_io': (688, 75),
}


def measured(engine, key, call):
    up0, down0 = engine.transfer_bytes()
    res = call()
    up1, down1 = engine.transfer_bytes()
    got = (up1 - up0, down1 - down0)
    print("    %r: %r," % (key, got))
    assert got == TRANSFERS[key], (key, got, TRANSFERS[key])
    return res


class Small:
    def __init__(self, engine):
        self.sig = SigWorld(engine, T, N, B5, 0x5A11)
        self.enc = EncWorld(engine, T, N, B5, 0x0E5C)
        gen = u8(o.g1_uncompressed(o.G1_GEN))[None]
        self.pk_sig = np.ascontiguousarray(engine.g1_mul(fr_rows(self.sig.sk), gen)[0][0])      # (N, 96): the public key shares
        self.pk_enc = np.ascontiguousarray(engine.g1_mul(fr_rows(self.enc.sk), gen)[0][0])


@pytest.fixture(scope="module")
def engine():
    """A context of this module's own, closed when the module ends: the byte counters start at zero, and nothing these calls
    allocate or set stays behind in the session's context for the modules that run later (tests/test_gpu_tables.py fills the HBM
    and expects an allocation to fail)."""
    from threshold_crypto_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def small(engine):
    return Small(engine)


@pytest.fixture(params=[True, False], ids=["checked", "unchecked"])
def checked(request, engine):
    engine.set_input_checks(request.param)
    yield request.param
    engine.set_input_checks(True)


def tag(checked):
    return "checked" if checked else "unchecked"


# ---- per message: the signature shares of B messages under N key shares ---------------------------------------------------
def test_verify_shares_rlc(engine, small, checked):
    w, pk = small.sig, small.pk_sig
    flat, off = pack_messages(w.msgs[:B3])
    pk_x = np.ascontiguousarray(np.tile(pk, (B3, 1)))
    h_x = np.ascontiguousarray(np.repeat(w.hashes[:B3], N, axis=0))
    for case, bad in (("clean", []), ("bad", [(2, 1)])):
        sh = np.ascontiguousarray(w.shares[:B3]).copy()
        for j, i in bad:
            sh[j, i] = w.shares[0, i]
        want = engine.verify_g2(pk_x, np.ascontiguousarray(sh.reshape(B3 * N, 192)), h_x).reshape(B3, N)
        assert [(int(j), int(i)) for j, i in zip(*np.nonzero(want == 0))] == bad
        assert bool(c.verify_g2(bytes(pk[1]), bytes(sh[2, 1]), bytes(w.hashes[2]))) == bool(want[2, 1])
        ok, nfb = measured(engine, "verify_shares_rlc %s %s" % (tag(checked), case), lambda: engine.verify_shares_rlc(pk, sh, flat, off, seed=SEED))
        assert ok.tolist() == want.tolist()
        assert nfb == _fallback([j for j, _ in bad], 1, B3)


# ---- grouped: many signatures under one key --------------------------------------------------------------------------------
GROUPED = (("clean", None, False, []), ("bad4", 4, False, [4]), ("bad0", 0, False, [0]), ("wrong_key", None, True, [0, 1, 2, 3, 4]))


@pytest.mark.parametrize("entry", ["verify_g2_rlc", "verify_sig_rlc"])
def test_grouped_signatures(engine, small, checked, entry):
    w = small.sig
    for case, bad, wrong_key, faults in GROUPED:
        pk = np.ascontiguousarray(w.commit[1 if wrong_key else 0])
        sig = w.want.copy()
        if bad is not None:
            sig[bad] = w.want[(bad + 1) % B5]
        if entry == "verify_g2_rlc":
            want = engine.verify_g2(pk, sig, w.hashes)
            run = lambda: engine.verify_g2_rlc(pk, sig, w.hashes, group=GROUP, seed=SEED)
        else:
            want = engine.verify_sig(pk, sig, w.flat, w.off)
            run = lambda: engine.verify_sig_rlc(pk, sig, w.flat, w.off, group=GROUP, seed=SEED)
        assert np.flatnonzero(want == 0).tolist() == faults
        assert bool(c.verify_g2(bytes(pk), bytes(sig[4]), bytes(w.hashes[4]))) == bool(want[4])
        ok, nfb = measured(engine, "%s %s %s" % (entry, tag(checked), case), run)
        assert ok.tolist() == want.tolist()
        assert nfb == _fallback(faults, GROUP, B5) == {"clean": 0, "bad4": 1, "bad0": 2, "wrong_key": 5}[case]


def test_ciphertext_verify_rlc(engine, small, checked):
    e = small.enc
    for case, faults in (("clean", []), ("bad4", [4]), ("bad0", [0]), ("every_group", [0, 2, 4])):
        w = e.w.copy()
        for j in faults:
            w[j] = e.w[(j + 1) % B5]
        want = engine.ciphertext_verify(e.u, e.v, e.off, w)
        assert np.flatnonzero(want == 0).tolist() == faults
        assert bool(c.ciphertext_verify(bytes(e.u[4]), bytes(e.v[int(e.off[4]):int(e.off[5])]), bytes(w[4]))) == bool(want[4])
        ok, nfb = measured(engine, "ciphertext_verify_rlc %s %s" % (tag(checked), case),
                           lambda: engine.ciphertext_verify_rlc(e.u, e.v, e.off, w, group=GROUP, seed=SEED))
        assert ok.tolist() == want.tolist()
        assert nfb == _fallback(faults, GROUP, B5) == {"clean": 0, "bad4": 1, "bad0": 2, "every_group": 5}[case]


# ---- records: ragged messages, keys named through a table -----------------------------------------------------------------------
REC_KEY_IDX = np.array([0, 1, 0], dtype=np.uint64)
REC_OFF = np.array([0, 2, 2, 3], dtype=np.uint64)
REC_JOB = [0, 0, 2]                                                        # the message / ciphertext of record r
REC_CASES = [("clean", None, False, []), ("bad_last", 2, False, [2]), ("bad_first", 0, False, [0])]
KEY_OUTSIDE_G1 = ("key_outside_g1", None, True, [1])                       # checked mode only


def records_fallback(faults):
    """n_fallback: every record of the groups that hold a fault"""
    groups = {REC_JOB[r] // GROUP for r in faults}
    return sum(1 for r in range(3) if REC_JOB[r] // GROUP in groups)


def on_device(*arrays):
    import torch
    dev = torch.device("cuda:0")
    return [torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).to(dev) for a in arrays]


@pytest.mark.parametrize("entry", ["verify_g2_records_rlc", "verify_sig_records_rlc"])
def test_records(engine, small, checked, entry):
    w = small.sig
    key_idx, rec_off, msg_of = REC_KEY_IDX, REC_OFF, REC_JOB
    hashes = np.ascontiguousarray(w.hashes[:3])
    flat, off = pack_messages(w.msgs[:3])
    for case, bad, outside, faults in REC_CASES + ([KEY_OUTSIDE_G1] if checked else []):
        pks = np.ascontiguousarray(small.pk_sig[:2]).copy()
        sigs = np.stack([w.shares[0, 0], w.shares[0, 1], w.shares[2, 0]])
        if bad is not None:
            sigs[bad] = w.shares[2 - msg_of[bad], 0]                       # key 0's signature of the OTHER message
        if outside:
            pks[1] = u8(o.g1_uncompressed(non_member_g1(random.Random(11))))
        pk_x, h_x = np.ascontiguousarray(pks[key_idx.astype(np.int64)]), np.ascontiguousarray(hashes[msg_of])
        want = engine.verify_g2(pk_x, sigs, h_x)
        assert np.flatnonzero(want == 0).tolist() == faults
        if not outside:                                                    # (the oracle's verify_g2 tests no membership)
            assert bool(c.verify_g2(bytes(pk_x[2]), bytes(sigs[2]), bytes(h_x[2]))) == bool(want[2])
        if entry == "verify_g2_records_rlc":
            run = lambda: engine.verify_g2_records_rlc(pks, key_idx, sigs, rec_off, hashes, group=GROUP, seed=SEED)
        else:
            run = lambda: engine.verify_sig_records_rlc(pks, key_idx, sigs, rec_off, flat, off, group=GROUP, seed=SEED)
        ok, nfb = measured(engine, "%s %s %s" % (entry, tag(checked), case), run)
        assert ok.tolist() == want.tolist()
        assert nfb == records_fallback(faults)


@pytest.mark.parametrize("entry", ["verify_g2_records_rlc", "verify_sig_records_rlc"])
def test_records_device_io(engine, small, entry):
    """the key table entry outside G1 with every operand in device memory: key_idx comes back to the host for the bad-group rule"""
    w = small.sig
    hashes = np.ascontiguousarray(w.hashes[:3])
    flat, off = pack_messages(w.msgs[:3])
    pks = np.ascontiguousarray(small.pk_sig[:2]).copy()
    pks[1] = u8(o.g1_uncompressed(non_member_g1(random.Random(11))))
    sigs = np.stack([w.shares[0, 0], w.shares[0, 1], w.shares[2, 0]])
    if entry == "verify_g2_records_rlc":
        call, rest = engine.verify_g2_records_rlc, (hashes,)
    else:
        call, rest = engine.verify_sig_records_rlc, (flat, off)
    want, want_nfb = call(pks, REC_KEY_IDX, sigs, REC_OFF, *rest, group=GROUP, seed=SEED)
    assert np.flatnonzero(np.asarray(want) == 0).tolist() == [1] and want_nfb == 2
    dev = on_device(pks, REC_KEY_IDX, sigs, REC_OFF, *rest)
    try:
        ok, nfb = measured(engine, "%s checked key_outside_g1 device_io" % entry, lambda: call(*dev, group=GROUP, seed=SEED))
        engine.sync()
        assert ok.cpu().numpy().tolist() == np.asarray(want).tolist() and nfb == want_nfb
    finally:
        engine.sync()


def dshare_records_inputs(small, bad, outside):
    """(pks, shares) of the three records: key 0 and key 1 for ciphertext 0, key 0 for ciphertext 2"""
    e = small.enc
    pks = np.ascontiguousarray(small.pk_enc[:2]).copy()
    shares = np.stack([e.shares[0, 0], e.shares[0, 1], e.shares[2, 0]])
    if bad is not None:
        shares[bad] = e.shares[2 - REC_JOB[bad], 0]                        # key 0's share of the OTHER ciphertext
    if outside:
        pks[1] = u8(o.g1_uncompressed(non_member_g1(random.Random(11))))
    return pks, shares


class DshareRecords:
    """the three ciphertexts of the decryption records cases, and their expansion to one ciphertext per record"""
    def __init__(self, engine, small):
        e = small.enc
        self.u, self.w = np.ascontiguousarray(e.u[:3]), np.ascontiguousarray(e.w[:3])
        self.v, self.off = np.ascontiguousarray(e.v[:int(e.off[3])]), np.ascontiguousarray(e.off[:4])
        self.vs = [bytes(e.v[int(e.off[j]):int(e.off[j + 1])]) for j in range(3)]
        hashes, st = engine.hash_g1_g2(self.u, self.v, self.off)
        assert not np.asarray(st).any()
        self.hashes = np.ascontiguousarray(hashes)
        self.u_x, self.w_x = np.ascontiguousarray(self.u[REC_JOB]), np.ascontiguousarray(self.w[REC_JOB])
        self.v_x, self.off_x = pack_messages([self.vs[j] for j in REC_JOB])

    def entry(self, engine, name):
        """(the entry, its operands behind rec_off)"""
        if name == "verify_decryption_share_records_rlc":
            return engine.verify_decryption_share_records_rlc, (self.u, self.v, self.off, self.w)
        return engine.verify_decryption_share_records_prehashed_rlc, (self.hashes, self.w)


DSHARE_ENTRIES = ["verify_decryption_share_records_rlc", "verify_decryption_share_records_prehashed_rlc"]


@pytest.fixture(scope="module")
def dshare(engine, small):
    return DshareRecords(engine, small)


@pytest.mark.parametrize("entry", DSHARE_ENTRIES)
def test_dshare_records(engine, small, dshare, checked, entry):
    d = dshare
    call, rest = d.entry(engine, entry)
    for case, bad, outside, faults in REC_CASES + ([KEY_OUTSIDE_G1] if checked else []):
        pks, shares = dshare_records_inputs(small, bad, outside)
        pk_x = np.ascontiguousarray(pks[REC_KEY_IDX.astype(np.int64)])
        want = engine.verify_decryption_share(pk_x, shares, d.u_x, d.v_x, d.off_x, d.w_x)
        assert np.flatnonzero(want == 0).tolist() == faults
        if not outside:                                                    # (the oracle's check tests no membership)
            assert bool(c.verify_decryption_share(bytes(pk_x[2]), bytes(shares[2]), bytes(d.u[2]), d.vs[2], bytes(d.w[2]))) == bool(want[2])
        ok, nfb = measured(engine, "%s %s %s" % (entry, tag(checked), case),
                           lambda: call(pks, REC_KEY_IDX, shares, REC_OFF, *rest, group=GROUP, seed=SEED))
        assert ok.tolist() == want.tolist()
        assert nfb == records_fallback(faults) == {"clean": 0, "bad_last": 1, "bad_first": 2, "key_outside_g1": 2}[case]


@pytest.mark.parametrize("entry", DSHARE_ENTRIES)
def test_dshare_records_device_io(engine, small, dshare, entry):
    """the key table entry outside G1 with every operand in device memory (test_records_device_io for the decryption shares)"""
    d = dshare
    call, rest = d.entry(engine, entry)
    pks, shares = dshare_records_inputs(small, None, True)
    want, want_nfb = call(pks, REC_KEY_IDX, shares, REC_OFF, *rest, group=GROUP, seed=SEED)
    assert np.flatnonzero(np.asarray(want) == 0).tolist() == [1] and want_nfb == 2
    dev = on_device(pks, REC_KEY_IDX, shares, REC_OFF, *rest)
    try:
        ok, nfb = measured(engine, "%s checked key_outside_g1 device_io" % entry, lambda: call(*dev, group=GROUP, seed=SEED))
        engine.sync()
        assert ok.cpu().numpy().tolist() == np.asarray(want).tolist() and nfb == want_nfb
    finally:
        engine.sync()


# ---- per ciphertext: the decryption shares of B ciphertexts under N key shares ------------------------------------------------
def test_verify_decryption_shares_rlc(engine, small, checked):
    e, pk = small.enc, small.pk_enc
    u, w = np.ascontiguousarray(e.u[:B3]), np.ascontiguousarray(e.w[:B3])
    v, off = np.ascontiguousarray(e.v[:int(e.off[B3])]), np.ascontiguousarray(e.off[:B3 + 1])
    vs = [bytes(e.v[int(e.off[j]):int(e.off[j + 1])]) for j in range(B3)]
    pk_x = np.ascontiguousarray(np.tile(pk, (B3, 1)))
    u_x, w_x = np.ascontiguousarray(np.repeat(u, N, axis=0)), np.ascontiguousarray(np.repeat(w, N, axis=0))
    v_x, off_x = pack_messages([vs[j] for j in range(B3) for _ in range(N)])
    for case, bad in (("clean", []), ("bad", [(2, 1)])):
        sh = np.ascontiguousarray(e.shares[:B3]).copy()
        for j, i in bad:
            sh[j, i] = e.shares[0, i]
        want = engine.verify_decryption_share(pk_x, np.ascontiguousarray(sh.reshape(B3 * N, 96)), u_x, v_x, off_x, w_x).reshape(B3, N)
        assert [(int(j), int(i)) for j, i in zip(*np.nonzero(want == 0))] == bad
        assert bool(c.verify_decryption_share(bytes(pk[1]), bytes(sh[2, 1]), bytes(u[2]), vs[2], bytes(w[2]))) == bool(want[2, 1])
        ok, nfb = measured(engine, "verify_decryption_shares_rlc %s %s" % (tag(checked), case),
                           lambda: engine.verify_decryption_shares_rlc(pk, sh, u, v, off, w, seed=SEED))
        assert ok.tolist() == want.tolist()
        assert nfb == _fallback([j for j, _ in bad], 1, B3)


# ---- DKG: the values of a part against its row commitment ----------------------------------------------------------------------
def test_dkg_verify_values_rlc(engine, checked):
    rnd = random.Random(0xD6)
    polys = [[rnd.randrange(1, o.R) for _ in range(2)] for _ in range(B3)]                     # degree 1
    rows = np.stack([np.asarray(engine.g1_commitment(fr_rows(p))[0]) for p in polys])         # (B, 2, 96)
    xs = np.array([[1, 2], [3, 4], [5, 6]], dtype=np.uint64)                                  # n = 2
    value = lambda j, k: o.poly_evaluate(polys[j], int(xs[j, k]))
    for case, bad in (("clean", []), ("bad", [(2, 1)])):
        vals = np.stack([fr_rows([value(j, k) for k in range(2)]) for j in range(B3)])
        for j, k in bad:
            vals[j, k] = fr_rows([value(j, k) + 1])[0]
        want = engine.dkg_verify_values(rows, xs, vals)
        assert [(int(j), int(k)) for j, k in zip(*np.nonzero(want == 0))] == bad
        pts = [o.g1_from_uncompressed(bytes(p), check=False) for p in rows[2]]
        val = int.from_bytes(bytes(vals[2, 1]), "little")
        assert (o.commitment_evaluate(pts, int(xs[2, 1])) == o.E1.mul(o.G1_GEN, val)) == bool(want[2, 1])
        ok, nfb = measured(engine, "dkg_verify_values_rlc %s %s" % (tag(checked), case), lambda: engine.dkg_verify_values_rlc(rows, xs, vals, SEED))
        assert ok.tolist() == want.tolist()
        assert nfb == _fallback([j for j, _ in bad], 1, B3)


# ---- the robust combiners: pass 1 over the first t + 1 present shares, pass 2 share by share or by bisection ---------------------
@pytest.mark.parametrize("bisect", [False, True], ids=["per_share", "bisect"])
@pytest.mark.parametrize("entry", ["sig", "sig_wire", "dec", "dec_wire"])
def test_robust_combiners(engine, small, checked, entry, bisect):
    sig, wire = entry.startswith("sig"), entry.endswith("wire")
    w = small.sig if sig else small.enc
    shares = np.ascontiguousarray(w.shares[:B3])
    want_out = None
    if sig:
        want_out = np.ascontiguousarray(w.want[:B3])
    if wire:
        comp, st = (engine.g2_compress if sig else engine.g1_compress)(np.ascontiguousarray(shares.reshape(B3 * N, shares.shape[2])))
        assert not np.asarray(st).any()
        shares = np.ascontiguousarray(np.asarray(comp).reshape(B3, N, -1))
        if sig:
            want_out, st = engine.g2_compress(want_out)
            assert not np.asarray(st).any()
    ident = IDENT2 if not wire else bytes([0xC0]) + bytes(95)
    if not sig:
        u, ww = np.ascontiguousarray(w.u[:B3]), np.ascontiguousarray(w.w[:B3])
        v, off = np.ascontiguousarray(w.v[:int(w.off[B3])]), np.ascontiguousarray(w.off[:B3 + 1])
    engine.set_blame_bisect(KEY if bisect else None)
    try:
        for case in ("clean", "bad"):
            plan = Plan(B3, N, T, shares)
            if case == "bad":
                plan.wrong(2, 1, other=0)                                  # inside S0 = {0, 1} of the last job
            want = plan.expect()
            assert want[2] == ((OK, [0, 2], [1], True) if case == "bad" else (OK, [0, 1], [], False))
            if sig:
                call = engine.combine_signatures_robust_wire if wire else engine.combine_signatures_robust
                run = lambda: call(w.commit, plan.shares, hashes=np.ascontiguousarray(w.hashes[:B3]), present=plan.present, seed=SEED)
            else:
                call = engine.decrypt_robust_wire if wire else engine.decrypt_robust
                run = lambda: call(w.commit, plan.shares, u, v, off, ww, present=plan.present)
            out, used, bad, st, nfb = measured(engine, "robust_%s %s %s %s" % (entry, "bisect" if bisect else "per_share", tag(checked), case), run)
            got = as_lists(used, bad, st, B3)
            for j in range(B3):
                assert got[j] == want[j][:3], (j, got[j], want[j])
                if sig:
                    assert bytes(out[j]) == (bytes(want_out[j]) if want[j][0] == OK else ident), j
                else:
                    lo, hi = int(off[j]), int(off[j + 1])
                    assert bytes(out[lo:hi]) == (w.plain[j] if want[j][0] == OK else bytes(hi - lo)), j
            assert nfb == sum(1 for x in want if x[3]) == (1 if case == "bad" else 0)
    finally:
        engine.set_blame_bisect(None)
