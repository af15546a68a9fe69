"""CPU checks of the byte layer of the device conformance suite (tests/device_conformance.py, ops 180 on): the references
themselves are pinned (a published ChaCha20 block; the two oracles agree on every malformed encoding), and the tables hold
the directed cases and the wave layouts that the per-wave loops of tc_hash.h need.  The ops themselves run in
tests/test_conformance_host.py (host leg) and tests/test_gpu_conformance.py (GPU leg), picked up from SPECS."""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import device_conformance as dc  # noqa: E402

o = dc.o
BYTE_OPS = sorted((op for op in dc.OPS if dc.OPS[op] >= dc.BYTE_OPS_FROM), key=lambda k: dc.OPS[k])


def test_chacha_reference_reproduces_the_published_block():
    """The all-zero key, counter 0: the first keystream block of ChaCha20 as published (76b8e0ad ... b2ee6586), through the
    oracle's block function, through chacha_words and through the oracle's ChaChaRng."""
    block = b"".join(w.to_bytes(4, "little") for w in o.chacha20_block([0] * 8, 0))
    assert block.hex() == dc.CHACHA_ZERO_KEY_BLOCK and block.hex().startswith("76b8e0ad") and block.hex().endswith("b2ee6586")
    assert dc.chacha_words([0] * 8, 0, 16) == list(o.chacha20_block([0] * 8, 0))
    rng = o.ChaChaRng(bytes(32))
    assert [rng.next_u32() for _ in range(16)] == dc.chacha_words([0] * 8, 0, 16) and rng.words_used == 16
    # the carry into word 13: block 2^32 - 1 is followed by block 2^32
    assert dc.chacha_words([1] * 8, (1 << 32) - 1, 32)[16:] == list(o.chacha20_block([1] * 8, 1 << 32))
    assert any(c.ctr == (1 << 32) - 1 and c.n > 16 for c in dc.table("CHACHA_WORDS"))
    assert {c.n for c in dc.table("CHACHA_WORDS")} >= set(dc.CHACHA_COUNTS)


def test_byte_layer_ops_and_lane_counts():
    assert len(BYTE_OPS) == 26 and set(BYTE_OPS) <= set(dc.SPECS)
    pair = {op for op in BYTE_OPS if dc.lanes(op) == 2}
    assert pair == {op for op in BYTE_OPS if dc.OPS[op] >= 200}
    assert all("2" in op for op in pair) and all(dc.lanes(op) in (1, 2) for op in BYTE_OPS)
    # at most three waves and a ragged tail, but for the tables that open with one whole wave per path -- and the combine job,
    # whose table IS its wave layouts: eleven waves, one per layout of its spec (test_wave_layout_of_the_combine_job)
    for op in BYTE_OPS:
        n, wave = len(dc.table(op)), 64 // dc.lanes(op)
        assert n % wave and n <= (12 if op == "JOB_COMBINE_SMALL_G2" else 5 if op in dc.LAYOUTS else 4) * wave, (op, n)


def test_malformed_encodings_have_one_verdict_in_both_oracles():
    """Every entry of the shared table of encodings: Oracle A's verdict (the reference of the decode ops) equals Oracle B's
    where B has the entry point -- the checked decode of both compressed forms, and the uncompressed parse of to_bytes."""
    import c_oracle as c
    counts = {}
    for g in (1, 2):
        for form in ("unc", "comp"):
            tbl = dc.byte_cases(g, form)
            counts[(g, form)] = len(tbl)
            fn = {(1, "comp"): c.g1_decompress, (2, "comp"): c.g2_decompress, (1, "unc"): c.g1_compress, (2, "unc"): c.g2_compress}[(g, form)]
            other = "unc" if form == "comp" else "comp"
            enc = {(1, "unc"): o.g1_uncompressed, (1, "comp"): o.g1_compressed, (2, "unc"): o.g2_uncompressed, (2, "comp"): o.g2_compressed}[(g, other)]
            for tag, kind, b in tbl:
                ok, p = dc.byte_ref(g, form, b)
                rc, out = fn(b)
                assert (rc == 0) == ok and rc in (0, 3), (g, form, tag, rc, ok)
                if ok:
                    assert out == enc(p), (g, form, tag)
            kinds = {k for _, k, _ in tbl}
            assert kinds >= ({"valid", "identity", "bad flags", "x out of range", "outside subgroup"} | ({"non-square"} if form == "comp" else set()))
            tags = " | ".join(t for t, _, _ in tbl)
            for need in ["top bits %d on a valid payload" % t for t in range(8)] + ["top bits %d on a zero payload" % t for t in range(8)] + \
                    ["stray bit 01 in byte 0", "stray bit 10 in byte 0", "in byte %d" % (dc.SIZE[(g, form)] - 1), "x = 0"]:
                assert need in tags, (g, form, need)
            # the uncompressed decode has no subgroup test, the compressed one rejects the same point
            outside = [b for _, k, b in tbl if k == "outside subgroup"][0]
            assert dc.byte_ref(g, form, outside)[0] == (form == "unc")
    assert counts == {(1, "unc"): 31, (1, "comp"): 31, (2, "unc"): 40, (2, "comp"): 38}, counts
    # both values of the sort bit decode to y and -y, and each encodes back to its input
    for g, dec, enc, E in ((1, o.g1_from_compressed, o.g1_compressed, o.E1), (2, o.g2_from_compressed, o.g2_compressed, o.E2)):
        a = [b for t, k, b in dc.byte_cases(g, "comp") if k == "valid" and t.startswith("top bits")][0]
        b = [b for t, _, b in dc.byte_cases(g, "comp") if t == "the other sort bit"][0]
        assert a[1:] == b[1:] and a[0] ^ b[0] == 0x20 and dec(a) == E.neg(dec(b)) and enc(dec(a)) == a and enc(dec(b)) == b
    # (0, 2) lies on E(Fq) outside G1
    assert o.E1.on_curve((0, 2)) and o.E1.mul((0, 2), o.R) is not None


def test_decode_tables_hold_the_shared_table_and_the_pairs():
    for op, g, form in (("G1_DECODE_UNCOMPRESSED", 1, "unc"), ("G1_DECODE_COMPRESSED", 1, "comp"), ("G2_DECODE_UNCOMPRESSED", 2, "unc"),
                        ("G2_DECODE_COMPRESSED", 2, "comp")):
        have = {c.b for c in dc.table(op)}
        assert all(b in have for _, _, b in dc.byte_cases(g, form)), op
    cases = dc.table("G2_DECODE_COMPRESSED_X2")
    kind_of = {dc.kind_encoding(k): k for k in dc.KINDS}
    kind_of_b = {dc.kind_encoding(k, -1): k for k in dc.KINDS}
    pairs = {(kind_of.get(c.encs[0]), kind_of_b.get(c.encs[1])) for c in cases if not c.null_b}
    assert pairs >= {(a, b) for a in dc.KINDS for b in dc.KINDS} and len(dc.KINDS) == 6
    assert sum(1 for c in cases if c.null_b and not dc.byte_ref(2, "comp", c.encs[0])[0]) >= 4
    stray = [c for c in cases if "identity with" in c.tag]
    assert len(stray) >= 6 and {("slot A" in c.tag) for c in stray} == {True, False}
    directed = [c for c in cases if not c.tag.startswith("random")]
    assert len(directed) == 36 + 6 + len(stray)


def test_hash_tables_hold_every_candidate_class_and_the_wave_layouts():
    """The bounded search finds a seed for every class 1 .. 10 (the accepted candidate is number 1 .. 10 of the stream), the
    directed cases hold each, and the tables are laid out as the per-wave loops need: whole waves on one path, then mixes."""
    cls = dc.seed_classes()
    assert all(cls.get(k) for k in range(1, 11)), sorted(cls)
    assert all(i < 300 for v in cls.values() for i in v)
    # the class is the number of candidates the oracle's own sampler tries
    for k in (1, 2, 10):
        stats = {}
        o.hash_g2(dc.hash_msg(cls[k][0]), stats)
        assert stats["attempts"] == k
        assert o.g2_uncompressed(o.hash_g2(dc.hash_msg(cls[k][0]))) == dc.hash_g2_ref(dc.hash_msg(cls[k][0]), 1)
    # fix = 0: the reference of G2_CLEAR_COFACTOR; [FR_COFACTOR_FIX] of it is the hash
    seed = dc.hash_seed(cls[2][0])
    assert o.E2.mul(dc.g2_random_ref(seed, 0), dc.COFACTOR_FIX) == dc.g2_random_ref(seed, 1)
    assert dc.g2_random_ref(seed, 1, 1) != dc.g2_random_ref(seed, 1)
    t = dc.table("G2_RANDOM_FROM_SEED")
    assert {dc.seed_class(c.seed) for c in t if c.tag.startswith("class")} == set(range(1, 11))
    assert {(c.fix, c.forced) for c in t} >= {(1, 0), (0, 0), (1, 1)}
    assert all(dc.seed_class(c.seed) == 1 for c in t[:32]) and all(dc.seed_class(c.seed) == 2 for c in t[32:64])
    assert {dc.seed_class(c.seed) for c in t[64:]} >= {1, 2, 3, 4, 9, 10}
    # x2: a wave in which exactly one slot of one pair needs ten candidates (slot B, then slot A), then the directed pairs
    t = dc.table("G2_RANDOM_FROM_SEED_X2")
    for w, slot in ((t[:32], 1), (t[32:64], 0)):
        slow = [(j, s) for j, c in enumerate(w) for s in (0, 1) if dc.seed_class(c.seeds[s]) != 1]
        assert len(slow) == 1 and slow[0][1] == slot and dc.seed_class(w[slow[0][0]].seeds[slot]) == 10
    assert {tuple(dc.seed_class(s) for s in c.seeds) for c in t[64:] if c.tag.startswith("pair")} == set(dc.X2_PAIRS)
    for op in ("HASH_G2_X2",):
        t = dc.table(op)
        got = {tuple(dc.seed_class(o.sha3_256(m)) for m in c.msgs) for c in t if c.tag.startswith("pair")}
        assert got == set(dc.X2_PAIRS) and any(c.null_b for c in t) and any(len(m) > 136 for c in t for m in c.msgs)
    assert {dc.seed_class(o.sha3_256(c.msg)) for c in dc.table("HASH_G2") if c.tag.startswith("class")} == set(range(1, 11))
    # SHA3: the lengths around the rate, a wave of one block, a wave of two, then 1, 2, 3 and 17 blocks mixed
    t = dc.table("SHA3_256")
    assert {len(c.msg) for c in t} >= set(dc.SHA3_LENGTHS) and {c.aux[1] for c in t} == {0, 1}
    assert all(dc.sha3_blocks(len(c.msg)) == 1 for c in t[:64]) and all(dc.sha3_blocks(len(c.msg)) == 2 for c in t[64:128])
    assert {dc.sha3_blocks(len(c.msg)) for c in t[128:192]} >= {1, 2, 3, 17}
    assert any(c.msg[-1:] == b"\x06" and len(c.msg) == 135 for c in t) and any(c.msg[-1:] == b"\x80" and len(c.msg) == 136 for c in t)
    assert any(c.msg == b"\xff" * 2240 for c in t)
    assert hashlib.sha3_256(b"").digest() == o.sha3_256(b"")
    # fq_random: a wave without a rejection in any of its lanes' eight draws, then none / one / three or more mixed
    t = dc.table("FQ_RANDOM")
    assert all(dc._fq_random_path(c) == "none" for c in t[:64])
    assert {dc._fq_random_path(c) for c in t[64:128]} >= {"none", "one", "many"}
    assert {c.n for c in t} == set(range(9))
    draws = dc.fq_draws(dc.fq_seed(0))
    assert [u for _, u, _ in draws] == sorted(u for _, u, _ in draws) and draws[-1][1] == 12 * (8 + sum(r for _, _, r in draws))
    # the lengths the issue names, present among the directed cases
    assert {len(c.data) for c in dc.table("XOR_WITH_HASH")} >= set(dc.XOR_LENS)
    assert {len(c.msg) for c in dc.table("HASH_G1_G2")} >= set(dc.HASH_LENS)
    t = dc.table("HASH_G1_G2_X2")
    oks = {tuple(dc.byte_ref(1, "unc", g1)[0] for g1, _ in c.ops) for c in t}
    assert oks == {(True, True), (True, False), (False, True), (False, False)}
    assert any({len(m) for _, m in c.ops} == {63, 65} for c in t) and any({len(m) for _, m in c.ops} == {64, 65} for c in t)
    assert {c.fix for c in t} == {0, 1} and any(c.null_b and not dc.byte_ref(1, "unc", c.ops[0][0])[0] for c in t)
    # an undecodable G1 operand in the internal form: 192 x ff, status 3
    bad = [b for k, b in dc._g1_operands() if k == "bad"][0]
    assert dc.hash_g1_g2_ref(bad, b"m", 0) == (3, b"\xff" * 192) and dc.hash_g1_g2_ref(bad, b"m", 1) == (3, o.g2_uncompressed(None))


def test_field_codec_tables_hold_the_edges():
    t = dc.table("FQ_FROM_BE48")
    assert {(c.v, c.top, c.mask) for c in t} >= {(v, top, m) for v in dc.BE_VALUES for top in range(8) for m in (0, 1)}
    assert dc.BE_VALUES == [0, 1, dc.P - 1, dc.P, dc.P + 1, (1 << 381) - 1]
    t = dc.table("FQ2_FROM_BE96")
    assert any(c.c[1] >= dc.P > c.c[0] for c in t) and any(c.c[0] >= dc.P > c.c[1] for c in t)
    assert any(c.tops[0] and c.mask and c.c[0] < dc.P and c.c[1] < dc.P for c in t)  # flag bits in c0's top byte, mask on: rejected
    t = dc.table("FQ2_LEX_LARGEST")
    vals = {dc.f2_in(c, 0) for c in t}
    assert vals >= {(v, 0) for v in (0, dc.HALF, dc.HALF + 1, dc.P - 1)} and any(c1 == dc.HALF for _, c1 in vals) and any(c1 == dc.HALF + 1 for _, c1 in vals)
    assert {dc.residue(c.slots[0].limbs) for c in dc.table("FQ_LEX_LARGEST")} >= {0, dc.HALF, dc.HALF + 1, dc.P - 1}
