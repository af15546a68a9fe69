"""GPU tests of batch verification over ragged input (tc_verify_g2_records_rlc_batch / tc_verify_sig_records_rlc_batch,
include/tc_amd.h): M messages, message m owning the records rec_off[m] .. rec_off[m + 1], record r = a signature
and the index of its key in a table of K keys.

Keys and signatures come from the library's own tc_g1_commitment_batch / tc_g2_mul_batch over fixed scalars (K = 7 keys, 12
messages, EVERY signature sk_i H_m made once per module); what a record must answer is computed by the C oracle's verify_g2
(once per distinct triple, cached for the module), and every case is also compared with tc_verify_g2_batch at pk_stride = 96 on
the expanded arrays.  A record whose index is outside the table has no key to expand: it stands in the expanded arrays with
96 bytes that do not decode, and its expected answer is 0 by construction -- like every record with a malformed operand."""
import random

import numpy as np
import pytest

import c_oracle as c
import tc_oracle as o
from threshold_crypto_amd.engine import pack_messages

pytestmark = pytest.mark.gpu
K, MSGS = 7, 12
SEED_A, SEED_B = bytes(range(32)), bytes(range(100, 132))
NO_KEY = np.full(96, 0xFF, dtype=np.uint8)


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def fr_rows(vals):
    return np.stack([u8(int(v % o.R).to_bytes(32, "little")) for v in vals])


class World:
    def __init__(self, engine):
        rnd = random.Random(0x7EC0)
        self.engine, self.rnd = engine, rnd
        self.sk = [rnd.randrange(1, o.R) for _ in range(K)]
        self.pks, st = engine.g1_commitment(fr_rows(self.sk))                                   # (K, 96)
        assert not np.asarray(st).any()
        self.msgs = [b"ragged message %d" % m for m in range(MSGS)]
        flat, off = pack_messages(self.msgs)
        self.hashes = engine.hash_g2(flat, off)                                                 # (MSGS, 192)
        out, st = engine.g2_mul(fr_rows(self.sk), self.hashes)                                  # [m, i] = sk_i H_m
        assert not np.asarray(st).any()
        self.sig = np.ascontiguousarray(out)
        self._oracle = {}

    def oracle(self, pk, sig, h):
        key = (bytes(pk), bytes(sig), bytes(h))
        if key not in self._oracle:
            self._oracle[key] = int(c.verify_g2(*key))
        return self._oracle[key]


@pytest.fixture(scope="module")
def world(engine):
    return World(engine)


class Case:
    """records of the first len(lens) messages: message m's k-th record is signed by key (m + k) % K unless `keys` says otherwise"""

    def __init__(self, world, lens, keys=None, msg_ids=None):
        self.w, self.lens, self.M = world, list(lens), len(lens)
        self.msg_ids = list(msg_ids) if msg_ids is not None else list(range(self.M))
        self.rec_off = np.zeros(self.M + 1, dtype=np.uint64)
        self.rec_off[1:] = np.cumsum(self.lens, dtype=np.uint64)
        self.R = int(self.rec_off[-1])
        self.msg_of = [m for m in range(self.M) for _ in range(self.lens[m])]
        self.key_idx = np.array([(m + k) % K if keys is None else keys(m, k) for m in range(self.M) for k in range(self.lens[m])], dtype=np.uint64)
        self.pks = world.pks.copy()
        self.hashes = np.ascontiguousarray(world.hashes[self.msg_ids])
        self.sigs = np.zeros((self.R, 192), dtype=np.uint8)
        for r in range(self.R):
            self.sigs[r] = world.sig[self.msg_ids[self.msg_of[r]], int(self.key_idx[r])]
        self.flat, self.off = pack_messages([world.msgs[i] for i in self.msg_ids])
        self.forced = {}                                   # record -> 0: malformed by construction (no oracle answer)

    def rec(self, m, k=0):
        return int(self.rec_off[m]) + k

    def group_records(self, group, recs):
        """records of the groups that hold any of `recs`"""
        group = group or 64
        groups = {self.msg_of[r] // group for r in recs}
        return [r for r in range(self.R) if self.msg_of[r] // group in groups]

    def expanded(self):
        pk = np.stack([self.pks[int(i)] if int(i) < K else NO_KEY for i in self.key_idx]) if self.R else np.zeros((0, 96), np.uint8)
        h = np.ascontiguousarray(self.hashes[self.msg_of]) if self.R else np.zeros((0, 192), np.uint8)
        return np.ascontiguousarray(pk), h

    def expect(self):
        pk, h = self.expanded()
        return np.array([self.forced[r] if r in self.forced else self.w.oracle(pk[r], self.sigs[r], h[r]) for r in range(self.R)], dtype=np.uint8)

    def run(self, engine=None, group=0, seed=SEED_A, key_idx="own"):
        eng = engine or self.w.engine
        kidx = self.key_idx if isinstance(key_idx, str) else key_idx
        ok, nfb = eng.verify_g2_records_rlc(self.pks, kidx, self.sigs, self.rec_off, self.hashes, group=group, seed=seed)
        return np.asarray(ok), nfb

    def check(self, engine=None, group=0, bad=(), seed=SEED_A):
        """the entry against the oracle, against the per-record path, and n_fallback against the records of the groups of `bad`"""
        eng = engine or self.w.engine
        want = self.expect()
        assert sorted(np.flatnonzero(want == 0).tolist()) == sorted(bad), "the case is not what the test meant to build"
        pk, h = self.expanded()
        per_record = np.asarray(eng.verify_g2(pk, self.sigs, h)) if self.R else np.zeros(0, np.uint8)
        ok, nfb = self.run(eng, group, seed)
        print("records %d, group %d: rejected %s, n_fallback %d" % (self.R, group, np.flatnonzero(ok == 0).tolist(), nfb))
        assert ok.tolist() == want.tolist()
        assert ok.tolist() == per_record.tolist()
        assert nfb == len(self.group_records(group, bad))
        return ok, nfb


RAGGED = [0, 1, 3, 1, 7, 0, 2]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [3, 1, 64])
def test_ragged_all_valid(world, group):
    """two full groups of three and a tail of one message at group = 3, an empty message in the first group and in the second"""
    case = Case(world, RAGGED)
    ok, nfb = case.check(group=group)
    assert ok.all() and nfb == 0


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["other_message", "other_key", "swapped"])
def test_one_forged_record(world, kind):
    case = Case(world, RAGGED)
    if kind == "other_message":                                   # message 2's record 1 carries its key's signature of message 3
        r = case.rec(2, 1)
        case.sigs[r] = world.sig[3, int(case.key_idx[r])]
        bad = [r]
    elif kind == "other_key":                                     # a valid signature of message 4 -- under the key next to the named one
        r = case.rec(4, 6)
        case.sigs[r] = world.sig[4, (int(case.key_idx[r]) + 1) % K]
        bad = [r]
    else:                                                         # two signatures of message 4 swapped between their keys
        a, b = case.rec(4, 0), case.rec(4, 5)
        case.sigs[[a, b]] = case.sigs[[b, a]]
        bad = [a, b]
    ok, nfb = case.check(group=3, bad=bad)
    # groups of three messages: {0, 1, 2} holds 4 records, {3, 4, 5} holds 8; only the forged record's group went record by record
    assert nfb == (4 if kind == "other_message" else 8)
    assert [r for r in range(case.R) if not ok[r]] == bad


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def test_cancelling_pair_is_rejected(world):
    """sigma_a + delta and sigma_b - delta on one message (delta = [d] H_m, a member of G2): the unweighted sum of the message's
    signatures is what it was, so an aggregate check would pass -- the weighted one rejects both records"""
    case = Case(world, RAGGED)
    m, a, b = 4, case.rec(4, 1), case.rec(4, 4)
    ka, kb = int(case.key_idx[a]), int(case.key_idx[b])
    d = world.rnd.randrange(1, o.R)
    out, st = world.engine.g2_mul(fr_rows([world.sk[ka] + d, world.sk[kb] - d]), world.hashes[m:m + 1])
    assert not np.asarray(st).any()
    lo, hi = case.rec(m), case.rec(m + 1)
    ones = np.broadcast_to(fr_rows([1])[0], (1, hi - lo, 32)).copy()
    before, st0 = world.engine.lincomb_g2(ones, np.ascontiguousarray(case.sigs[lo:hi][None]))
    case.sigs[a], case.sigs[b] = out[0, 0], out[0, 1]
    after, st1 = world.engine.lincomb_g2(ones, np.ascontiguousarray(case.sigs[lo:hi][None]))
    assert not np.asarray(st0).any() and not np.asarray(st1).any()
    assert bytes(np.asarray(before)[0]) == bytes(np.asarray(after)[0]) != bytes(o.g2_uncompressed(None))
    assert world.engine.g2_subgroup_check(np.ascontiguousarray(case.sigs[[a, b]])).all()
    ok, nfb = case.check(group=3, bad=[a, b])
    assert nfb == 8


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def _non_member_g2(rnd):
    while True:
        P = o.g2_get_point_from_x((rnd.randrange(o.Q), rnd.randrange(o.Q)), True)
        if P is not None and o.E2.mul(P, o.R) is not None:
            return u8(o.g2_uncompressed(P))


# (a point outside G2 is only told apart in checked-input mode: no case with the checks off)
MALFORMED = [(kind, checked) for kind in ("sig_undecodable", "sig_non_member", "key_undecodable", "index_K", "index_max") for checked in (True, False)
             if checked or kind != "sig_non_member"]


@pytest.mark.parametrize("kind,checked", MALFORMED)
def test_one_malformed_operand(world, kind, checked):
    eng = world.engine
    case = Case(world, RAGGED)
    if kind == "sig_undecodable":
        bad = [case.rec(4, 2)]
        case.sigs[bad[0], 100] ^= 1                              # not on the curve
    elif kind == "sig_non_member":
        bad = [case.rec(2, 0)]
        case.sigs[bad[0]] = _non_member_g2(random.Random(5))
    elif kind == "key_undecodable":
        case.pks[3, 50] ^= 1                                     # every record that names key 3, and only those
        bad = [r for r in range(case.R) if int(case.key_idx[r]) == 3]
        assert len(bad) >= 2 and len({case.msg_of[r] for r in bad}) >= 2
    else:
        bad = [case.rec(4, 3)]
        case.key_idx[bad[0]] = K if kind == "index_K" else 2 ** 64 - 1
    for r in bad:
        case.forced[r] = 0
    eng.set_input_checks(checked)
    try:
        ok, nfb = case.check(group=3, bad=bad)
    finally:
        eng.set_input_checks(True)
    assert [r for r in range(case.R) if not ok[r]] == bad


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_without_an_index_array_record_r_uses_key_r(world):
    """K = R = M = 9, one record per message, distinct keys: the result is tc_verify_sig_batch's with pk_stride = 96"""
    eng = world.engine
    n = 9
    sk = [world.rnd.randrange(1, o.R) for _ in range(n)]
    pks, _ = eng.g1_commitment(fr_rows(sk))
    msgs = [b"one record each %d" % m for m in range(n)]
    flat, off = pack_messages(msgs)
    hashes = eng.hash_g2(flat, off)
    allsig, _ = eng.g2_mul(fr_rows(sk), hashes)
    sigs = np.ascontiguousarray(np.stack([allsig[m, m] for m in range(n)]))
    rec_off = np.arange(n + 1, dtype=np.uint64)
    for forged in ([], [2, 7]):
        s = sigs.copy()
        for r in forged:
            s[r] = allsig[r, (r + 1) % n]
        want = np.asarray(eng.verify_sig(pks, s, flat, off))
        assert [r for r in range(n) if not want[r]] == forged
        for r in range(n):
            assert world.oracle(pks[r], s[r], hashes[r]) == want[r]
        assert np.asarray(eng.verify_g2(pks, s, hashes)).tolist() == want.tolist()
        ok, nfb = eng.verify_sig_records_rlc(pks, None, s, rec_off, flat, off, group=4, seed=SEED_A)
        assert np.asarray(ok).tolist() == want.tolist() and nfb == (8 if forged else 0)      # groups {0..3}, {4..7}, {8}
        ok, nfb = eng.verify_g2_records_rlc(pks, None, s, rec_off, hashes, group=4, seed=SEED_A)
        assert np.asarray(ok).tolist() == want.tolist() and nfb == (8 if forged else 0)
    with pytest.raises(ValueError):
        eng.verify_g2_records_rlc(pks[:8], None, sigs, rec_off, hashes)                       # K < R without an index array


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_dense_input_equals_the_share_matrix_entry(world):
    """N = 5 keys x B = 6 messages, every record present, one forged share: the ok matrix of tc_verify_shares_rlc_batch"""
    eng = world.engine
    N, B = 5, 6
    case = Case(world, [N] * B, keys=lambda m, k: k)
    case.pks = np.ascontiguousarray(world.pks[:N])
    r = case.rec(3, 2)
    case.sigs[r] = world.sig[3, 4]
    shares = np.ascontiguousarray(case.sigs.reshape(B, N, 192))
    matrix, nfb_m = eng.verify_shares_rlc(case.pks, shares, case.flat, case.off, seed=SEED_A)
    matrix = np.asarray(matrix)
    assert nfb_m == 1 and [tuple(x) for x in np.argwhere(matrix == 0)] == [(3, 2)]
    want = case.expect()
    assert want.reshape(B, N).tolist() == matrix.tolist()
    for group in (1, 4):
        ok, nfb = eng.verify_g2_records_rlc(case.pks, case.key_idx, case.sigs, case.rec_off, case.hashes, group=group, seed=SEED_A)
        assert np.asarray(ok).reshape(B, N).tolist() == matrix.tolist() and nfb == N * group                 # the forged share's group: message 3 alone, or the messages 0 .. 3
    ok, nfb = eng.verify_sig_records_rlc(case.pks, case.key_idx, case.sigs, case.rec_off, case.flat, case.off, group=1, seed=SEED_B)
    assert np.asarray(ok).reshape(B, N).tolist() == matrix.tolist() and nfb == N
    pk, h = case.expanded()
    assert np.asarray(eng.verify_g2(pk, case.sigs, h)).reshape(B, N).tolist() == matrix.tolist()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
LONG = [130, 0, 1, 3, 4, 5, 33]


@pytest.fixture(scope="module")
def long_cases(world):
    """segment lengths that make a job span more than a wave of lane pairs, leave padded chunk places and put items of very
    different length in one wave, over K = 5 repeated keys: all valid, and the LAST record of the 130-segment forged"""
    good = Case(world, LONG, keys=lambda m, k: (m + k) % 5)
    forged = Case(world, LONG, keys=lambda m, k: (m + k) % 5)
    r = forged.rec(0, 129)
    forged.sigs[r] = world.sig[0, (int(forged.key_idx[r]) + 1) % 5]
    want = forged.expect()                                       # the oracle's 176 answers, once for the module
    assert good.expect().all() and np.flatnonzero(want == 0).tolist() == [r]
    return good, forged, r


def _long(eng, long_cases):
    good, forged, r = long_cases
    ok, nfb = good.check(eng, group=2)
    assert ok.all() and nfb == 0
    ok, nfb = forged.check(eng, group=2, bad=[r])
    assert nfb == 130 and [i for i in range(forged.R) if not ok[i]] == [r]   # the group {0, 1}: 130 + 0 records


def test_long_and_odd_segments_in_one_launch(world, long_cases):
    _long(world.engine, long_cases)


@pytest.mark.parametrize("parts", [1, 64])
def test_long_and_odd_segments_with_the_split_forced(long_cases, parts):
    """TC_RECORDS_PARTS: the smallest and the largest split (64 lanes per message in G1, 32 lane pairs per group in G2)"""
    from conftest import engine_with_env
    with engine_with_env(TC_RECORDS_PARTS=parts) as eng:
        _long(eng, long_cases)


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_forms_agree(world):
    import torch
    eng = world.engine
    case = Case(world, RAGGED)
    r = case.rec(3, 0)
    case.sigs[r] = world.sig[2, int(case.key_idx[r])]
    want, _ = case.check(group=3, bad=[r])
    other_seed, nfb = case.run(group=3, seed=SEED_B)
    assert other_seed.tolist() == want.tolist() and nfb == 8
    ok, nfb = eng.verify_sig_records_rlc(case.pks, case.key_idx, case.sigs, case.rec_off, case.flat, case.off, group=3, seed=SEED_A)
    assert np.asarray(ok).tolist() == want.tolist() and nfb == 8
    dev = torch.device("cuda:0")
    t8 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)
    try:
        ok, nfb = eng.verify_g2_records_rlc(t8(case.pks), t64(case.key_idx), t8(case.sigs), t64(case.rec_off), t8(case.hashes), group=3, seed=SEED_A)
        eng.sync()
        assert ok.cpu().numpy().tolist() == want.tolist() and nfb == 8
        ok, nfb = eng.verify_sig_records_rlc(t8(case.pks), t64(case.key_idx), t8(case.sigs), t64(case.rec_off), t8(case.flat), t64(case.off), group=3,
                                             seed=SEED_A)
        eng.sync()
        assert ok.cpu().numpy().tolist() == want.tolist() and nfb == 8
    finally:
        eng.sync()


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_empty_inputs(world):
    eng = world.engine
    none8 = lambda n: np.zeros((0, n), dtype=np.uint8)
    ok, nfb = eng.verify_g2_records_rlc(world.pks, np.zeros(0, np.uint64), none8(192), np.zeros(1, np.uint64), none8(192), seed=SEED_A)
    assert np.asarray(ok).shape == (0,) and nfb == 0
    # every message empty: nothing is written, through the C ABI with a guarded ok buffer
    import ctypes
    from threshold_crypto_amd import _native
    lib = _native.load()
    M = 5
    rec_off = np.zeros(M + 1, dtype=np.uint64)
    hashes = np.ascontiguousarray(world.hashes[:M])
    guard = np.full(8, 0xA5, dtype=np.uint8)
    nfb = ctypes.c_uint64(77)
    rc = lib.tc_verify_g2_records_rlc_batch(eng._ctx, world.pks.ctypes.data, K, None, None, rec_off.ctypes.data, hashes.ctypes.data, M, 2, SEED_A,
                                            guard.ctypes.data, ctypes.byref(nfb))
    assert rc == _native.TC_OK and nfb.value == 0 and (guard == 0xA5).all()
    nfb = ctypes.c_uint64(77)
    rc = lib.tc_verify_g2_records_rlc_batch(eng._ctx, None, 0, None, None, None, None, 0, 0, None, None, ctypes.byref(nfb))
    assert rc == _native.TC_OK and nfb.value == 0
    # a malformed offset array gets the answer a malformed `off` gets
    from threshold_crypto_amd.engine import TcError
    case = Case(world, [1, 2])
    for broken in ([1, 2, 4], [0, 2, 1]):
        rc = lib.tc_verify_g2_records_rlc_batch(eng._ctx, case.pks.ctypes.data, K, case.key_idx.ctypes.data, case.sigs.ctypes.data,
                                                np.array(broken, dtype=np.uint64).ctypes.data, case.hashes.ctypes.data, 2, 0, SEED_A,
                                                guard.ctypes.data, None)
        assert rc == _native.TC_ERR_INVALID_ARG and (guard == 0xA5).all()
    with pytest.raises(TcError):
        eng.hash_g2(np.zeros(16, np.uint8), np.array([0, 9, 4], dtype=np.uint64))            # ... the same code


# ---- the typed interface -----------------------------------------------------------------------------------------------------------
def test_public_key_verify_records_batch(world):
    """PublicKey.verify_records_batch: per-message lists of (key, signature) pairs, equal keys deduplicated into the table"""
    from threshold_crypto_amd import api
    case = Case(world, RAGGED)
    forged = case.rec(6, 1)
    case.sigs[forged] = world.sig[6, (int(case.key_idx[forged]) + 2) % K]
    want = case.expect()
    assert np.flatnonzero(want == 0).tolist() == [forged]
    keys = [api.PublicKeyShare(world.pks[i], _trusted=True) for i in range(K)]
    records = [[(keys[int(case.key_idx[r])] if r % 2 else api.PublicKey(world.pks[int(case.key_idx[r])], _trusted=True),
                 api.SignatureShare(case.sigs[r], _trusted=True)) for r in range(case.rec(m), case.rec(m + 1))] for m in range(case.M)]
    msgs = [world.msgs[m] for m in range(case.M)]
    got = api.PublicKey.verify_records_batch(records, msgs, engine=world.engine, seed=SEED_A, group=3)
    assert [len(row) for row in got] == RAGGED
    assert [x for row in got for x in row] == [bool(x) for x in want]
    assert api.PublicKey.verify_records_batch([[] for _ in msgs], msgs, engine=world.engine) == [[] for _ in msgs]
    with pytest.raises(ValueError):
        api.PublicKey.verify_records_batch(records[:-1], msgs, engine=world.engine)
