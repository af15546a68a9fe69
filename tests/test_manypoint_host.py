"""CPU leg of the many-point conformance suite (tests/manypoint_conformance.py): the two-stage MSM (G2 and G1) and the comb
signer.

(a) tests/device/manypoint.hip -- the product's k_msm.hip and k_comb.hip plus the harness entries -- cross-compiles for
    gfx950 with the product's flags.
(b) The models are checked against the oracle: the recodings decode back to the scalar, the entry tables from the affine
    group law are the multiples the walk uses, the walk on multiples agrees with the walk on the oracle's group law
    (sum AND special-case verdict), msm_part tiles [0, n).
(c) Every directed job's claim holds in the model ("this part meets a special case", "this merge round doubles / cancels /
    meets the identity"), and every random filler job is shown to meet none, at every legal parts.
(d) The host leg (tests/device/manypoint_host.cpp, g++ -DTC_BOUND_CHECK: the header routines the kernels call) runs the
    full case tables of the GPU leg through the same checkers, so tables, models and checkers are proven before a GPU run.
(e) The ragged sums of the records verifier (k_rec_*): the model's rec_part is the library's, the tables have the shapes the
    ragged forms need, every directed segment hits what it claims, and the host leg runs every table at every parts.
(f) The paired ragged sums (k_rec_*_g1_pair): the halves of a segment are different samples under the same scalars, a directed
    segment has its special case in one half and a partner that meets nothing in the other, no directed segment is left out,
    and the host leg (rec_pair_chunk / _place / _lane / _out as the kernels use them, the negated half) runs every table.
(g) The G1 comb of the decryption shares: the model of the doubling-free pass (only the scalar 0 meets a special case), the
    directed placements each case claims per share (by the kernel's lane order), and the host leg at share = 1 .. 8.
(h) Blame by bisection (k_blame.hip): tests/device/manypoint_blame.hip cross-compiles; the tables hold what the kernels' text needs
    (ragged waves, leaf numbers across 2^32, dead slots first / last / in mid-wave, directed digit rows at lane 0 / last / middle,
    the head of ranges, no empty range); the suite's leaf encoder and decoder agree; every directed range meets what it claims and
    random ones meet only the identities of their empty parts; the host leg runs leaves, ladders, range sums and the chain.
"""
import ctypes
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import manypoint_conformance as mp  # noqa: E402

dc, o, R, X, X2 = mp.dc, mp.o, mp.R, mp.X, mp.X2

G2_FULL = [8, 9, 13, 68]
G2_SHORT = [1, 5, 64]
G1_FULL = [8, 9, 13, 68]
G1_SHORT = [(1, 80), (10, 32), (70, 32)]
SHARED = [(10, "good"), (10, "job0 even"), (10, "job0 >= r"), (70, "good"), (70, "job0 >= r")]
COMB = [(3, 5), (8, 5), (9, 5), (24, 5), (30, 5), (30, 70)]


def test_manypoint_kernels_cross_compile_for_gfx950():
    lib = mp.build_device()
    assert os.path.getsize(lib) > 0
    with open(lib, "rb") as f:
        text = f.read()
    for name in (b"mp_msm_g2", b"mp_msm_g1", b"mp_comb", b"mp_rec_sum", b"mp_rec_gather_keys",
                 b"k_rec_tables_g2", b"k_rec_ladder_g2", b"k_rec_tables_g1", b"k_rec_ladder_g1", b"k_rec_gather_keys",
                 b"mp_rec_sum_pair", b"mp_comb_g1", b"mp_g1_mul_gather", b"k_rec_tables_g1_pair", b"k_rec_ladder_g1_pair", b"k_comb_tables_g1",
                 b"k_comb_decrypt", b"k_g1_mul_gather"):
        assert name in text, name  # the entries of the harness and the ragged, paired and G1 comb kernels they reach


@pytest.fixture(scope="module")
def host():
    return mp.load(mp.build_host(), "mph_")


def test_stand_alone_program_of_the_host_leg_passes():
    r = subprocess.run([mp.build_host_main()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


# ---- (b) the models ---------------------------------------------------------------------------------------------------
def test_msm_part_tiles_the_shares(host):
    """For every tested (n, parts): the ranges tile [0, n), none is empty, trips = ceil(n / parts) covers the longest --
    in the model and in tc_msm.h msm_part."""
    out = (ctypes.c_size_t * 3)()
    shapes = {(w, n) for w, ns in ((2, G2_FULL + G2_SHORT + [2, 3, 4, 128]), (1, G1_FULL + [1, 10, 70, 256])) for n in ns}
    for w, n in sorted(shapes):
        legal = mp.legal_parts(w, n)
        assert legal[0] == 1 and all(p & (p - 1) == 0 and (p == 1 or 4 * p <= n) for p in legal)
        for p in legal:
            nxt = 0
            for g in range(p):
                s0, s1, trips = mp.msm_part(n, g, p)
                host["lib"].mph_msm_part(ctypes.c_size_t(n), ctypes.c_size_t(g), ctypes.c_size_t(p), out)
                assert (s0, s1, trips) == tuple(out), (n, g, p)
                assert s0 == nxt and s1 > s0 and s1 - s0 in (trips, trips - 1) and trips == -(-n // p)
                nxt = s1
            assert nxt == n
    assert mp.legal_parts(2, 128)[-1] == 32 and mp.legal_parts(1, 256)[-1] == 64 and mp.legal_parts(2, 127)[-1] == 16
    # the launcher's own choice for the suite's shapes is one of the legal values
    assert [mp.launcher_parts(2, n, 37) for n in (4, 8, 13, 68)] == [1, 2, 2, 16] and mp.launcher_parts(2, 128, 3) == 32
    assert [mp.launcher_parts(1, n, 70) for n in (1, 10, 70)] == [1, 2, 16] and mp.launcher_parts(1, 256, 3) == 64


def test_buffer_sizes_match_the_product(host):
    out = (ctypes.c_size_t * 4)()
    for n, B in ((1, 1), (9, 37), (68, 70)):
        host["lib"].mph_sizes(ctypes.c_size_t(n), ctypes.c_size_t(B), out)
        s4 = 4 * ((n + 3) // 4)
        assert list(out) == [B * s4 * 8 * 64 * 4, B * 65 * s4, B * s4 * 8 * 32 * 4, B * 65 * 8 * 64 * 4]


def test_recodings_decode_back_to_the_scalar():
    rnd = random.Random(7)
    assert mp.sac_cols([5, 7, 0, 1 << 63]) == dc.sac_model([5, 7, 0, 1 << 63])[:3]
    for w in (1, 2):
        ks = mp.edge_scalars(w) + [rnd.randrange(R) for _ in range(30)]
        for k in ks:
            codes, flip, fits = mp.codes_of(w, k, 64 if w == 2 else 128)
            assert fits and flip == (k % 2 == 0) and len(codes) == 65
            assert mp.codes_value(w, codes) == (R - k if flip else k), hex(k)
        nb = 16 if w == 2 else 32
        for _ in range(30):
            k = mp.short_scalar(w, nb, rnd)
            codes, flip, fits = mp.codes_of(w, k, nb)
            assert fits and not flip and len(codes) == (nb if w == 2 else nb // 2) + 1 and mp.codes_value(w, codes) == k
        assert mp.codes_of(w, 1, nb, padding=True) == mp.codes_of(w, 1, nb)
        for k in (2, R - 1, (1 << nb) * (X if w == 2 else X2) + 1):
            codes, flip, fits = mp.codes_of(w, k, nb)
            assert not fits and mp.codes_value(w, codes) == 1
    # the G1 edge list holds scalars with k1 even (flipped) and with the top column at entry 3
    tops = [mp.g1_codes(k)[0][-1] for k in mp.edge_scalars(1)]
    assert 3 in tops and 0 in tops and any(k % 2 == 0 for k in mp.edge_scalars(1))
    assert 1 + (1 << 80) * X2 < R  # (the longest short scalars of the suite are scalars)


def test_entry_tables_and_walks_agree_with_the_oracle():
    """psi = [x] and phi' = [x^2]: the entries from the affine group law are the multiples the integer walk uses; the walk
    on multiples and the walk on the oracle's group law give the same sum and the same special-case verdict, for generic
    jobs and for jobs built on an exception."""
    rnd = random.Random(13)
    for w in (1, 2):
        a = mp.pool(w)[5]
        for flip in (False, True):
            assert mp.entry_points(w, a, flip) == [mp.gmul(w, m) for m in mp.entry_mults(w, a, flip)]
        assert mp.gmul(w, a) == mp.E[w].mul(mp.GEN[w], a) and mp.gmul(w, R - 1) == mp.E[w].neg(mp.GEN[w])
        assert mp.entry_points(w, 0) == [None] * 8
        n, nbits = 5, 64 if w == 2 else 128
        jobs = [mp.random_job(w, n, nbits, rnd)] + [j for j in mp.directed_jobs(w, n, nbits, rnd) if j.claim]
        verdicts = set()
        for job in jobs:
            case = mp.MsmCase(w, n, 1, nbits, [job], [1])
            codes, flips, ok = case.share_codes(job)
            assert ok
            mults = [mp.entry_mults(w, job.a[s], flips[s]) for s in range(n)]
            points = [mp.entry_points(w, job.a[s], flips[s]) for s in range(n)]
            for s0, s1 in ((0, n), (1, 3)):
                m, sp = mp.walk_part(w, mults, codes, s0, s1)
                pt, sp2 = mp.walk_part_points(w, points, codes, s0, s1)
                assert pt == mp.gmul(w, m) and sp == sp2, job.tag
                assert m == sum(job.a[s] * job.k[s] for s in range(s0, s1)) % R
                verdicts.add(sp)
        assert verdicts == {False, True}
    assert mp.merge_events([5, 5, 7, R - 7]) == (10, [(0, 0, "equal"), (0, 1, "equal"), (0, 2, "opposite"), (0, 3, "opposite"), (1, 0, "identity"),
                                                      (1, 1, "identity"), (1, 2, "identity"), (1, 3, "identity")])
    assert mp.merge_events([1, 2, 3, 4]) == (10, [])


def test_comb_model():
    """The doubling-free pass in units of the message point: it gives k for every key.  For a valid key the recoding never
    sets fix (d0 = k' mod 2 is odd because |x| is even).  Of tiny keys, keys next to r and small digit vectors the model
    finds exactly one that meets a special case over a point other than the identity: the key 0 (it runs as r, and the last
    addition is P = -Q); the other way onto the safe ladder is a message at the identity."""
    case = mp.comb_case(3, 5)
    small = [c0 + c1 * X + c2 * X2 + c3 * X ** 3 for c0 in range(4) for c1 in range(3) for c2 in range(2) for c3 in range(2)]
    for k in case.keys + list(range(64)) + [R - k for k in range(1, 64)] + small:
        if k < R:
            flip, fix, special, m = mp.comb_model(k)
            assert (R - m if flip else m) % R == k and not fix and special == (k == 0), hex(k)
    assert {0, 1, 2, R - 1} <= set(case.keys) and any(k >= R for k in case.keys)
    for n, B in COMB:
        c = mp.comb_case(n, B)
        flat = [i for row in c.idx for i in row]
        assert any(i >= c.N for i in flat) and {0, None} <= set(c.msgs) and (B > 8 or any(n % s for s in c.shares if s))
        assert {c.keys[i] for i in flat if i < c.N} >= ({0, 1, 2, R - 1, R} if B == 5 and n >= 8 else {0, 1})


# ---- (c) the claims ---------------------------------------------------------------------------------------------------
def _all_msm_cases():
    cases = [mp.msm_case(2, n, 64, 37) for n in G2_FULL] + [mp.msm_case(2, n, 16, 37) for n in G2_SHORT]
    cases += [mp.msm_case(1, n, 128, 70) for n in G1_FULL] + [mp.msm_case(1, n, nb, 70) for n, nb in G1_SHORT]
    cases += [mp.top_case(2), mp.top_case(1)]
    return cases


def test_directed_jobs_hit_what_they_claim_and_random_ones_hit_nothing():
    seen = set()
    for case in _all_msm_cases():
        assert not mp.check_claims(case), case.tag
        assert not getattr(case, "left_out", []), (case.tag, case.left_out)
        tags = [j.tag for j in case.jobs]
        seen |= {t.split(" of part")[0].split(" at round")[0].split(" at the start")[0] for t in tags}
        assert sum(j.random for j in case.jobs) >= (3 if case.B > 3 else 1), case.tag
        if case.B > 8:  # adversarial jobs share waves with ordinary ones; the head of the batch is ordinary
            head = 8 if case.w == 2 else 32
            assert all(j.random for j in case.jobs[:head]) and not all(j.random for j in case.jobs[head:])
            assert case.B % (32 if case.w == 2 else 64) and case.B > (32 if case.w == 2 else 64)
    assert seen >= {"identity first", "identity in the middle", "identity: every share", "equal shares", "P and -P, equal scalars,",
                    "all shares equal", "equal shares across a part boundary", "equal shares at the masked position", "merge equal",
                    "merge opposite", "merge identity", "status not OK on entry", "undecodable point", "scalar = r", "largest short digits",
                    "even short scalar", "digit with bit nbits set", "random"}, seen
    # a later round of the tree is reached where parts >= 4
    big = [j.claim["merge"] for c in _all_msm_cases() for j in c.jobs if j.claim and "merge" in j.claim]
    assert {r for r, _ in big} >= {0, 3, 4, 5} and {k for _, k in big} == {"equal", "opposite", "identity"}


# ---- (d) the host leg over the full case tables -----------------------------------------------------------------------------
def _run_case(host, case):
    first = None
    for parts in case.parts:
        if parts == 0:
            continue  # the launcher's own choice: the device leg
        res = mp.run_msm(host, case, parts)
        if first is None or not all((a == b).all() for a, b in zip(res, first)):  # (equal bytes need no second decoding)
            bad = mp.check_msm(case, parts, res)
            assert not bad, "\n".join(bad[:12])
        if first is None:
            first = res
        assert all((a == b).all() for a, b in zip(res, first)), (case.tag, parts)


@pytest.mark.parametrize("n", G2_FULL)
def test_host_g2_msm_full_scalars(host, n):
    _run_case(host, mp.msm_case(2, n, 64, 37))


@pytest.mark.parametrize("n", G2_SHORT)
def test_host_g2_msm_short_scalars(host, n):
    _run_case(host, mp.msm_case(2, n, 16, 37))


@pytest.mark.parametrize("n,need", [(2, -1), (3, -1), (4, -1), (3, 0), (3, 5)])
def test_host_g2_msm_filter(host, n, need):
    case = mp.filter_case(n, need)
    taken = [case.taken(j) for j in range(case.B)]
    assert (any(taken) and not all(taken)) if need else not any(taken)
    _run_case(host, case)


@pytest.mark.parametrize("w", [2, 1])
def test_host_msm_largest_parts(host, w):
    _run_case(host, mp.top_case(w))


@pytest.mark.parametrize("n", G1_FULL)
def test_host_g1_msm_full_scalars(host, n):
    _run_case(host, mp.msm_case(1, n, 128, 70))


@pytest.mark.parametrize("n,nbits", G1_SHORT)
def test_host_g1_msm_short_scalars(host, n, nbits):
    _run_case(host, mp.msm_case(1, n, nbits, 70))


@pytest.mark.parametrize("n,variant", SHARED)
def test_host_g1_msm_shared_set(host, n, variant):
    """A failing job 0 must not change the table set it builds for everybody: jobs 1 .. B-1 still equal the oracle."""
    case = mp.shared_case(n, variant)
    st = case.ref()[0]
    assert st.count(mp.OK) >= case.B - 6 and (st[0] == mp.OK) == (variant == "good") and st[5] == st[40] == st[67] == mp.INVALID
    _run_case(host, case)


@pytest.mark.parametrize("n,B", COMB)
def test_host_comb(host, n, B):
    case = mp.comb_case(n, B)
    first = None
    for share in case.shares:
        if share == 0:
            continue
        res = mp.run_comb(host, case, share)
        if first is None or not all((a == b).all() for a, b in zip(res, first)):
            bad = mp.check_comb(case, share, res)
            assert not bad, "\n".join(bad[:12])
        if first is None:
            first = res
        assert all((a == b).all() for a, b in zip(res, first))


# ---- the ragged sums (k_rec_*; tc_records.h) --------------------------------------------------------------------------------
def test_rec_part_of_the_model_tiles_a_segment_as_the_library_does(host):
    """For every length of the tables and every parts: the model's rec_part is tc_records.h's, the ranges tile [0, len) in
    order, a part holds trips or trips - 1 records (EMPTY ones where len < parts), and trips = ceil(len / parts)."""
    out = (ctypes.c_uint64 * 3)()
    lens = sorted({n for w, kind in mp.REC_TABLES for n in mp.rec_case(w, kind).lens} | {0, 1, 2, 3, 4, 5, 7, 8, 9, 33, 64, 65, 130})
    for n in lens:
        for p in mp.REC_PARTS[1]:
            nxt, empty = 0, 0
            for g in range(p):
                s0, s1, trips = mp.rec_part(n, g, p)
                host["lib"].mph_rec_part(ctypes.c_uint64(n), ctypes.c_size_t(g), ctypes.c_size_t(p), out)
                assert (s0, s1, trips) == tuple(out), (n, g, p)
                assert s0 == nxt and s1 >= s0 and trips == -(-n // p) and (s1 - s0 in (trips, trips - 1) or s1 == s0)
                nxt, empty = s1, empty + (s1 == s0)
            assert nxt == n and empty == max(p - n, 0), (n, p)
    sz = (ctypes.c_size_t * 3)()
    host["lib"].mph_rec_sizes(ctypes.c_uint64(7), sz)
    assert list(sz) == [7 * 4 * 8 * 64 * 4, 7 * 4 * 8 * 32 * 4, 7 * 4 * 65]


def test_rec_tables_have_the_shapes_the_ragged_forms_need():
    for w in (1, 2):
        case = mp.rec_case(w, "short")
        most = mp.MAX_PARTS[w]
        assert case.J == mp.REC_J > most and case.J % most and case.records < 512 and case.lens[:2] == [0, 0]
        assert set(case.lens) >= {0, 1, 2, 3, 4, 5, 7, 8, 9, 33, 64, 65, 130}
        assert case.parts == [p for p in (1, 2, 4, 8, 16, 32, 64) if p <= most] + [3, 2 * most]
        assert all(s.random for s in case.segs[:16]) and case.lens[2:4] == [130, 1]  # whole waves of random segments first
        directed = sum(not s.random for s in case.segs)
        assert directed >= 20
        for i in range(16, 16 + 4 * (directed // 3), 4):  # then three directed segments and a random one
            assert [s.random for s in case.segs[i:i + 4]] == [False, False, False, True], i
        assert case.nbits == mp.REC_NBITS[w] and mp.rec_case(w, "full").nbits == mp.REC_FULL[w]
        st = mp.rec_case(w, "fail first").ref()[0]
        assert mp.rec_case(w, "fail first").lens[:3] == [0, 3, 0] and st[:3] == [mp.OK, mp.INVALID, mp.OK] and mp.NOT_ENOUGH in st
        assert mp.rec_case(w, "no segment").J == 0 and mp.rec_case(w, "all empty").chunks == 0 and mp.rec_case(w, "one record").lens == [1]
    assert all(k == 1 for s in mp.rec_case(2, "unit").segs for k in s.k)
    pks, idx, want = mp.gather_case()
    assert {0, mp.GATHER_K - 1, mp.GATHER_K, 1 << 32, (1 << 64) - 1} <= set(idx) and len(idx) == 71 and (71 * 6) % 64 and len(want) == 72 * 96


def test_directed_segments_hit_what_they_claim_and_random_ones_hit_nothing():
    seen, merges = set(), set()
    for w, kind in mp.REC_TABLES:
        case = mp.rec_case(w, kind)
        assert not mp.check_rec_claims(case), case.tag
        assert not case.left_out, (case.tag, case.left_out)
        if kind in ("short", "unit", "full"):
            tags = {s.tag for s in case.segs}
            seen |= tags
            assert tags >= {"equal neighbours", "P and -P", "P, -P, Q", "identity alone", "identity first, and first of part 2/4", "identity in mid-part",
                            "opposite halves", "undecodable first record", "undecodable last record", "status not OK on entry"}, case.tag
            claims = [c for s in case.segs if isinstance(s.claim, list) for c in s.claim]
            merges |= {(w, c["parts"]) + c["merge"] for c in claims if "merge" in c}
            st = case.ref()[0]
            for j, s in enumerate(case.segs):  # a failing segment sits between segments that are OK
                if st[j] != mp.OK:
                    assert st[j - 1] == mp.OK and (j + 1 == case.J or st[j + 1] == mp.OK or not case.segs[j + 1].random), (case.tag, j)
    assert seen >= {"even scalar", "scalar that is not short", "scalar = r", "digit with bit nbits set", "merge opposite at round 0 of parts 2"}, seen
    assert merges >= {(2, 32, 4, "opposite"), (1, 64, 5, "opposite"), (2, 32, 4, "equal"), (2, 2, 0, "equal"), (2, 8, 2, "opposite"), (1, 64, 0, "identity")}


def _run_rec(host, case):
    first = None
    for parts in case.parts:
        res = mp.run_rec(host, case, parts)
        if first is None or not all((a == b).all() for a, b in zip(res, first)):  # (equal bytes need no second decoding)
            bad = mp.check_rec(case, parts, res)
            assert not bad, "\n".join(bad[:12])
        if first is None:
            first = res
        assert all((a == b).all() for a, b in zip(res, first)), "%s: parts = %d and parts = %d leave different bytes" % (case.tag, parts, case.parts[0])


@pytest.mark.parametrize("w,kind", mp.REC_TABLES)
def test_host_rec_sum(host, w, kind):
    """Every legal parts gives the bytes of parts = 1 -- outputs, statuses, tables, codes, guards --, an illegal one too."""
    _run_rec(host, mp.rec_case(w, kind))


def test_host_rec_gather_keys(host):
    got, want = mp.run_gather(host)
    assert got == want


# ---- the paired ragged sums (k_rec_*_g1_pair; tc_records.h rec_pair_*) -------------------------------------------------------
def test_pair_tables_have_the_shapes_the_paired_forms_need():
    case = mp.pair_case("short")
    assert case.nbits == mp.PAIR_NBITS == 32 and case.J == mp.REC_J > 64 and case.J % 64 and case.lens[:16] == mp.REC_HEAD
    assert case.parts == [1, 2, 4, 8, 16, 32, 64, 3, 128] and mp.pair_case("full").nbits == 128 and mp.pair_case("full").J == 27
    assert all(p.random for p in case.pairs[:16])
    for kind in ("short", "full"):
        case = mp.pair_case(kind)
        tags = {p.tag for p in case.pairs}
        want = {"equal neighbours in a", "P and -P in b", "P and -P in a", "identity alone in b", "identity in mid-part in b", "opposite halves in a",
                "undecodable first record in a", "undecodable last record in b", "undecodable first record in both", "scalar = r in a",
                "status not OK on entry in a"} | ({"even scalar in b", "scalar that is not short in a"} if kind == "short" else set())
        assert tags >= want, (kind, want - tags)
        st, out = case.ref()
        for j, p in enumerate(case.pairs):
            a, b = p.half
            assert a.k == b.k and len(a.a) == len(b.a)
            if not p.random or case.lens[j] > 1:  # the halves are different samples: a common error cannot hide in equal inputs
                assert a.a != b.a or not case.lens[j], (kind, j)
            if st[j] != mp.OK:                    # a failing segment sits between segments that are OK, identities in both rows
                assert st[j - 1] == mp.OK and (j + 1 == case.J or st[j + 1] == mp.OK or not case.pairs[j + 1].random), (kind, j)
                assert out[2 * j] == out[2 * j + 1] == mp.enc(1, None)
        by_tag = {p.tag: j for j, p in enumerate(case.pairs)}
        # a failure in ONE half fails the segment: the other half alone is valid
        j = by_tag["undecodable first record in a"]
        assert not case.half[0].valid(j) and case.half[1].valid(j) and st[j] == mp.INVALID
        j = by_tag["undecodable last record in b"]
        assert case.half[0].valid(j) and not case.half[1].valid(j) and st[j] == mp.INVALID
        j = by_tag["scalar = r in a"]
        assert not case.half[0].valid(j) and not case.half[1].valid(j)
        # B is the identity while A is not: the negated half keeps the canonical encoding
        j = by_tag["P and -P in b"]
        assert st[j] == mp.OK and out[2 * j + 1] == bytes([0x40]) + bytes(95) and out[2 * j] != out[2 * j + 1]
        j = by_tag["P and -P in a"]
        assert st[j] == mp.OK and out[2 * j] == bytes([0x40]) + bytes(95) and out[2 * j + 1][0] != 0x40
    # -B_j: the x of B_j, the other y
    case = mp.pair_case("one record")
    b = case.pairs[0].half[1]
    pt = mp.gmul(1, b.a[0] * b.k[0] % R)
    assert case.ref()[1][1] == mp.enc(1, (pt[0], mp.P - pt[1]))
    st = mp.pair_case("fail first").ref()[0]
    assert mp.pair_case("fail first").lens[:3] == [0, 3, 0] and st[:3] == [mp.OK, mp.INVALID, mp.OK] and mp.NOT_ENOUGH in st
    assert mp.pair_case("no segment").J == 0 and mp.pair_case("all empty").chunks == 0
    assert mp.pair_case("all empty").ref()[1] == [bytes([mp.POISON]) * 96] * 10  # chunks == 0: nothing is written


def test_directed_pairs_hit_what_they_claim_and_random_halves_hit_nothing():
    for kind in mp.PAIR_TABLES:
        case = mp.pair_case(kind)
        assert not mp.check_pair_claims(case), case.tag
        assert not case.left_out, (case.tag, case.left_out)
        for j, p in enumerate(case.pairs):  # the partner of a directed half is a random one, with claims of its own to meet nothing
            assert p.random == all(h.random for h in p.half) and (p.random or sum(h.random for h in p.half) == 1), (case.tag, j)
    claims = [(h, c) for p in mp.pair_case("short").pairs for h in (0, 1) if isinstance(p.half[h].claim, list) for c in p.half[h].claim]
    assert {h for h, _ in claims} == {0, 1} and {c["merge"] for _, c in claims if "merge" in c} >= {(5, "opposite"), (5, "equal"), (0, "identity")}


@pytest.mark.parametrize("kind", mp.PAIR_TABLES)
def test_host_rec_sum_pair(host, kind):
    """Every parts gives the bytes of parts = 1: A_j and -B_j, statuses, both halves' tables and codes, the guards."""
    case = mp.pair_case(kind)
    mp.sweep(host, case, mp.run_rec_pair, mp.check_rec_pair, case.parts, "parts")


# ---- the G1 comb (k_comb_tables_g1 / k_comb_decrypt; tc_comb_g1.h) --------------------------------------------------------------
def test_comb_g1_model_and_cases():
    """The doubling-free pass in units of u gives k for every valid key, and of the key table only the scalar 0 meets a special
    case over a point other than the identity (the guarded fallback).  Every case holds what COMB1_CLAIMS says it holds, at the
    share it names, by the kernel's own lane order."""
    case = mp.comb1_case(9, 70)
    assert case.keys[:12] == [0, 1, 2, 3, 4, 5, X2, X2 - 1, X2 + 1, R - 1, R, (1 << 256) - 1] and len(case.keys) == case.N == 16
    for k in case.keys + list(range(6, 40)) + [R - k for k in range(2, 40)]:
        if k < R:
            m, special = mp.comb1_model(k)
            assert m == k and special == (k == 0), hex(k)
    for n, B in mp.COMB1_SHAPES:
        c = mp.comb1_case(n, B)
        assert c.shares == list(range(9)) and {0, None} <= set(c.u)
        for share, kinds in mp.COMB1_CLAIMS[(n, B)].items():
            assert kinds <= mp.comb1_events(c, share), (n, B, share, kinds - mp.comb1_events(c, share))
        flat = [i for row in c.idx for i in row]
        if n >= 9:
            assert {c.N, 1 << 32, (1 << 64) - 1, mp.K_ZERO, mp.K_R, mp.K_BIG} <= set(flat)
            assert any(row.count(7) >= n - 4 for row in c.idx) and (n > 13 or any(row == sorted(row, reverse=True) and len(set(row)) == n for row in c.idx))
    # B = 70, n = 9: at share 4 wave 2 mixes cnt = 4 with cnt = 1 and wave 3 has 18 live lanes; at share 8 cnt = 8 sits beside cnt = 1
    assert -(-9 // 4) * 70 == 210 and 210 - 192 == 18 and -(-9 // 8) * 70 == 140
    assert case.u[64] == 0 and case.u[69] is None and case.checked == [0, 63, 64, 69]
    # the launcher's own rule never leaves share = 1 at these shapes: the suite forces it
    assert all(n * B <= 131072 for n, B in mp.COMB1_SHAPES)


@pytest.mark.parametrize("n,B", mp.COMB1_SHAPES)
def test_host_comb_g1(host, n, B):
    case = mp.comb1_case(n, B)
    mp.sweep(host, case, mp.run_comb1, mp.check_comb1, case.shares[1:], "share")  # (share = 0, the launcher's choice: the device leg)


# ---- blame by bisection (k_blame.hip; tc_blame_jobs.h) --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bhost():
    return mp.load_blame(mp.build_host(), "mph_")


def test_blame_kernels_cross_compile_for_gfx950():
    lib = mp.build_device_blame()
    with open(lib, "rb") as f:
        text = f.read()
    for name in (b"mp_blame_leaves", b"mp_blame_range_sum", b"mp_blame_chain", b"mp_blame_ladder", b"mp_blame_sum_parts", b"k_blame_seed",
                 b"k_blame_leaves", b"k_blame_range_sum", b"k_mp_blame_ladder"):
        assert name in text, name


def test_blame_tables_have_the_shapes_the_kernels_need():
    for w in (1, 2):
        W = mp.WAVE_LEAVES[w]
        assert [s[0] for s in mp.LEAVES_SHAPES[:5]] == [1, 33, 64, 65, 130] and {s[1] for s in mp.LEAVES_SHAPES} >= {0, 2 ** 32 - 3}
        assert mp.LEAVES_SHAPES[5:] == [(130, 0, 52, False), (130, 7 * 52, 52, True)]
        cases = [mp.leaves_case(w, *s) for s in mp.LEAVES_SHAPES]
        assert {c.call for c in cases} == {0, 1, 2 ** 40 + 3}
        c = cases[4]   # n = 130 with a live array: every kind first, last and in the middle of a wave
        first = {c.kind(r) for r in range(0, 130, W)}
        last = {c.kind(r) for r in list(range(W - 1, 130, W)) + [129]}
        mid = {c.kind(v * W + W // 2 - 3 + 3 * j) for v in range(130 // W) for j in range(3)}
        assert first >= set(c.KINDS) and last >= set(c.KINDS) and mid >= set(c.KINDS), (first, last, mid)
        if w == 2:   # both of a wave's last lane pairs
            assert all(c.kind(v * W + W - 2) != "point" and c.kind(v * W + W - 1) != "point" for v in range(4))
        assert c.leaf0 < 2 ** 32 < c.leaf0 + c.n and c.live[21] == 0xff and c.live[20] == 0 and c.a[20] is None
        st = c.ref()
        assert st[3][20] == 0 and st[3][21] == 0xff and st[3][130] == mp.POISON
        cleared = [r for r in range(130) if c.live[r] and not st[3][r]]
        assert cleared and all(c.kind(r) == "bad" for r in cleared) and sum(m != 0 for m in st[1]) > 100
        assert cases[5].live is None and {cases[5].kind(r) for r in range(130)} == {"point", "identity", "bad"}
        assert {cases[6].kind(r) for r in range(130)} == {"point", "identity", "bad", "not live"} and len(cases[6].a) == 52
        # the ladder rows
        lc = mp.ladder_case(w)
        assert lc.T == 69 and [d for d in mp.LADDER_DIGITS if d[0] % 2 == 0] == []
        directed = {s: lc.rows[s] for s in lc.spots}
        assert len(directed) == 21 and {0, W - 1, (lc.T // W) * W} <= set(directed) and any(abs(s % W - W // 2) <= 1 for s in directed)
        for d in mp.LADDER_DIGITS:
            assert sorted((a != 0, live) for a, live, dd in directed.values() if dd == d) == [(False, 1), (True, 0), (True, 1)], d
        assert len({r[2] for r in lc.rows}) == 7 + mp.LADDER_RANDOM and all(r[2][0] & 1 for r in lc.rows)
        for v in range(0, lc.T, W):   # the rows of a wave all differ
            assert len(set(lc.rows[v:v + W])) == len(lc.rows[v:v + W])
        # the range sums
        rc = mp.range_case(w)
        n = len(rc.items)
        assert n >= 100 and all(n % (W // p) for p in mp.REC_PARTS[w] if W // p > 1)
        assert [it.hi - it.lo for it in rc.items[:13]] == mp.BLAME_HEAD and all(it.random for it in rc.items[:16])
        head = rc.items[:13]
        assert any(it.lo % 2 == 0 and it.lo for it in head) and any(it.lo % 2 for it in head) and any(it.lo == 0 for it in head)
        assert any(it.hi == rc.N and it.lo for it in head) and [it.job for it in head[:4]] == [1, 0, 1, 0]
        assert all(0 <= it.lo < it.hi <= rc.N and it.job < rc.F for it in rc.items)          # no empty range: outside the contract
        for i in range(16, 16 + 4 * 15, 4):
            assert [it.random for it in rc.items[i:i + 4]] == [False, False, False, True], i
        assert {it.tag for it in rc.items} >= {"all identities", "one live leaf, first", "one live leaf, last", "one live leaf, in the middle",
                                               "equal neighbours", "P, -P", "P, -P, Q", "halves that cancel in the last round",
                                               "back at the identity in mid-part, and on"}
        want = rc.ref()
        ident = mp.enc(w, None)
        for it, o_ in zip(rc.items, want):
            assert (o_ == ident) == (it.tag in ("all identities", "P, -P", "halves that cancel in the last round")), it.tag
        assert rc.leaves.size == rc.F * rc.N * mp.LEAF_ROWS[w] * 16 and len(set(rc.m[:2 * rc.N])) == 2 * rc.N
        assert mp.BLAME_PARTS[w] == [0] + [p for p in (1, 2, 4, 8, 16, 32, 64) if p <= W] + [3, 2 * W]


def test_leaf_words_decode_to_their_point():
    """The test's own leaf encoder against the leaf decoder: both representatives, a random Z, the identity as (0, 1, 0)."""
    rnd = random.Random(11)
    for w in (1, 2):
        for m in [0] + mp.pool(w)[:6]:
            bad = []
            row = mp.leaf_words(w, m, rnd)
            assert len(row) == mp.LEAF_ROWS[w] * 16 and mp.leaf_point(w, row, "leaf", bad) == mp.gmul(w, m) and not bad
        rows = [mp.leaf_words(w, mp.pool(w)[0], rnd) for _ in range(8)]
        assert len({tuple(r) for r in rows}) == 8   # (another Z, another representative)
        assert any(dc.value(r[:14]) >= mp.P for r in rows) and any(dc.value(r[:14]) < mp.P for r in rows)
        bad = []
        mp.leaf_point(w, mp.leaf_words(w, 5, rnd)[:-1] + [1], "leaf", bad)
        assert bad


def test_blame_items_hit_what_they_claim_and_random_ones_hit_nothing():
    for w in (1, 2):
        case = mp.range_case(w)
        assert not mp.check_blame_claims(case), case.tag
        assert sum(bool(it.claims) for it in case.items) == 45
    # the model itself: parts beyond the terms leave parts without a term, whose identities are explained, and only those
    total, ev, mev, unexplained = mp.blame_item_model([5, 7, 11], 0, 3, 8)
    assert total == 23 and not ev and not unexplained and {e[2] for e in mev} == {"identity"}
    assert mp.blame_item_model([5, 0, 11], 0, 3, 1)[1] == [(0, 1, "term identity")]
    assert mp.blame_item_model([5, 0, 11], 0, 3, 4)[3]                                # the identity of a part WITH a term is not
    assert mp.blame_item_model([5, 5], 0, 2, 2)[3] == [(0, 0, "equal"), (0, 1, "equal")]


@pytest.mark.parametrize("w,shape", [(w, s) for w in (1, 2) for s in mp.LEAVES_SHAPES])
def test_host_blame_leaves(bhost, w, shape):
    case = mp.leaves_case(w, *shape)
    bad = mp.check_blame_leaves(case, mp.run_blame_leaves(bhost, case))
    assert not bad, "\n".join(bad[:12])


@pytest.mark.parametrize("w", [1, 2])
def test_host_blame_ladder_at_chosen_digits(bhost, w):
    case = mp.ladder_case(w)
    bad = mp.check_blame_ladder(case, mp.run_blame_ladder(bhost, case))
    assert not bad, "\n".join(bad[:12])


@pytest.mark.parametrize("w", [1, 2])
def test_host_blame_range_sum(bhost, w):
    """Every parts gives the oracle's bytes for every item -- parts beyond the terms, 3 and twice the maximum (run as 1) too."""
    case = mp.range_case(w)
    mp.sweep(bhost, case, mp.run_blame_range, mp.check_blame_range, mp.BLAME_PARTS[w][1:], "parts")  # (0, blame_sum_parts: the device leg)


@pytest.mark.parametrize("w", [1, 2])
def test_host_blame_chain(bhost, w):
    case = mp.chain_case(w)
    mp.sweep(bhost, case, mp.run_blame_chain, mp.check_blame_chain, case.parts[1:], "parts")


def test_blame_sum_parts_model_is_the_documented_rule():
    """(the product's blame_sum_parts is compared with this model in the GPU leg: it lives in k_blame.hip)"""
    assert len(mp.SUM_PARTS_TABLE) == 2 * 2 * 7 * 3
    assert mp.blame_sum_parts_model(1, 101, 130, 0) == 64 and mp.blame_sum_parts_model(2, 101, 130, 0) == 32
    assert mp.blame_sum_parts_model(1, 1, 127, 256) == 32 and mp.blame_sum_parts_model(1, 65536, 200, 1) == 1
    assert mp.blame_sum_parts_model(2, 65536, 200, 256) == 1 and mp.blame_sum_parts_model(1, 65536, 200, 256) == 1
    assert [mp.blame_sum_parts_model(1, 1, n, 0) for n in (1, 2, 3, 4, 127, 128, 200)] == [1, 1, 1, 2, 32, 64, 64]
