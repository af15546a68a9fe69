"""Host leg of the DKG kernel conformance suite (tests/dkg_conformance.py): proves the case tables, the models and the checkers on
tests/device/dkg_kernels_host.cpp (the header routines of tc_dkg.h under g++ -DTC_BOUND_CHECK) before any GPU time is spent.  The
GPU leg (tests/test_gpu_dkg_kernels.py) runs the same tables through the shipped kernels.

(a) the stand-alone program of the host leg passes; (b) the models state what they claim: the signed windows of the fixed-base
multiplication (every directed scalar has its digit, the table entries a canonical scalar can reach), sum_part / wsum_slice_part
against the header's, the P / -P pairs inside a lane and across the xor tree, the Horner events of the directed commitments;
(c) the host leg passes every checker over the case tables; (d) every checker notices a spoiled buffer."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dkg_conformance as dk  # noqa: E402

o, R = dk.o, dk.R
HOST_PARTS = [p for p in dk.PARTS if p]  # (0 is the launcher's rule: the device leg only)


@pytest.fixture(scope="module")
def host():
    return dk.load(dk.build_host(), "dkh_")


def _ok(bad):
    assert not bad, "\n".join(bad[:12])


def _spoiled(check, res, index, *args, at=3):
    """The checker must notice one flipped byte in buffer `index` of a passing result."""
    res = dict(res) if isinstance(res, dict) else list(res)
    buf = res[index].copy()
    flat = buf.view(np.uint8).reshape(-1)
    flat[min(len(flat) - 1, at)] ^= 0x10
    res[index] = buf
    assert check(*args, res), "a spoiled %s went unnoticed" % (index,)


def test_stand_alone_program_of_the_host_leg_passes():
    r = subprocess.run([dk.build_host_main()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


# ---- (b) the models ---------------------------------------------------------------------------------------------------
def test_signed_window_model():
    """The recoding is exact, its digits lie in -7 .. 8 (a magnitude 8 is never negative), every directed scalar has the digit it is
    listed for, and the entries a canonical scalar reaches are all but (63, 8): r's leading nibbles are 0x73."""
    case = dk.fb_case()
    reached = set()
    for k in case.scalars:
        digits, carry = dk.fb_digits(k)
        assert dk.fb_value(digits, carry) == k
        assert all(0 <= m <= 8 and not (neg and m == 8) for m, neg in digits)
        if k < R:
            assert carry == 0
            reached |= {(w, m) for w, (m, _) in enumerate(digits) if m}
    for k, what in case.directed:
        digits, _ = dk.fb_digits(k)
        if what.startswith("digit"):
            sign, w = what.split()[1], int(what.split()[-1])
            assert digits[w] == (int(sign[1:]), sign[0] == "-"), what
            if sign[0] == "-":
                assert digits[w + 1] == (1, False), what  # the carry went up
        if what.startswith("entry"):
            assert digits[63] == (int(what[-2]), False)
    chain, _ = dk.fb_digits((1 << 80) - 7)
    assert chain[0] == (7, True) and all(d == (0, True) for d in chain[1:20]) and chain[20] == (1, False)
    assert dk.fb_digits(0xfff9 << 236)[0][63] == (1, False)
    for w in (0, 31, 62):
        assert {(w, m) for m in range(1, 9)} <= reached
    assert {(63, m) for m in range(1, 8)} <= reached and (63, 8) not in reached
    # window 63 holds 8 only with the top nibble 7 and a carry out of window 62, i.e. a top byte >= 0x78 > 0x73
    for top in range(0x74):
        for rest in (0, (1 << 248) - 1):
            k = (top << 248) | rest
            if k < R:
                assert dk.fb_digits(k)[0][63][0] <= 7
    assert dk.fb_digits(0x789 << 244)[0][63] == (8, False) and (0x78 << 248) >= R  # (the smallest such top byte, with a carry from below)
    assert dk.fb_digits(R)[1] == 0 and dk.fb_digits((1 << 256) - 1)[1] == 1


def test_sum_part_models_against_the_header(host):
    out = np.zeros(2, dtype=np.uint64)
    for n in dk.SUM_NS + [3]:
        for parts in (1, 2, 4, 8, 16, 32, 64):
            nxt = 0
            for g in range(parts):
                host["lib"].dkh_sum_part(n, 0, 0, g, parts, out.ctypes.data_as(dk.ctypes.c_void_p))
                assert (int(out[0]), int(out[1])) == dk.sum_part(n, g, parts) and out[0] == nxt
                nxt = int(out[1])
            assert nxt == n
            for slices in (1, 2, 3, 5, 64, n):
                if slices > n:
                    continue
                nxt = 0
                for s in range(slices):
                    for g in range(parts):
                        host["lib"].dkh_sum_part(n, s, slices, g, parts, out.ctypes.data_as(dk.ctypes.c_void_p))
                        assert (int(out[0]), int(out[1])) == dk.slice_part(n, s, slices, g, parts) and out[0] == nxt
                        nxt = int(out[1])
                assert nxt == n


def test_opposite_pairs_meet_inside_a_lane_and_in_the_xor_tree():
    """Every case with two terms or more has a P, -P pair that lies in one lane at one parts value and in two lanes at another (the
    adjacent pair at the head of 130 terms stays in lane 0 at every parts value; the mirrored one splits)."""
    for n in dk.SUM_NS:
        case = dk.sum_case(n, "included")
        split = False
        for a, b in case.pairs:
            assert (case.m[a][1] + case.m[b][1]) % R == 0 and case.m[a][1]
            together = {parts: dk.lane_of(n, a, parts) == dk.lane_of(n, b, parts) for parts in (1, 2, 4, 8, 16, 32, 64)}
            assert together[1], (n, a, b)
            split = split or not all(together.values())
        assert split == (n >= 2), n
    assert dk.sum_case(130, "included").pairs == [(0, 1), (64, 65)]
    assert dk.lane_of(130, 64, 2) == 0 and dk.lane_of(130, 65, 2) == 1  # mirrored across the split of two lanes


def test_directed_commitments_meet_their_horner_events():
    for case in dk.rows_directed_cases():
        _, st, events = case.ref()
        for t in range(case.lanes):
            coeffs, x = case.lane(t)
            kind = case.jobs[0 if case.form == 0 else (t // case.n if case.form == 2 else t // (case.degree + 1))]
            if "random" in kind.tag:
                assert not events[t] and st[t] == dk.OK
        tags = {c.tag for c in case.jobs}
        seen = {e for t in range(case.lanes) for e in events[t] if case.lane(t)[1] == 2}
        if any("c = -[x] res" in t for t in tags):
            assert "cancel" in seen, case.tag
        if any("c = [x] res" in t or "and c = [x] res" in t for t in tags):
            assert "double" in seen, case.tag
        if any("off-curve" in t for t in tags):
            assert dk.INVALID in st and dk.OK in st, case.tag
    for b in (dk.off_curve(), dk.BAD):
        with pytest.raises(o.DecodeError):
            o.g1_from_uncompressed(b)


def test_parts_and_slices_rules():
    """What the launcher's rules give at the shapes of the suite (the device leg compares the harness's answer with these models)."""
    assert dk.g1_sum_parts_model(9, 130, 1, 0) == 32 and dk.g1_sum_parts_model(9, 130, 1, 8) == 8 and dk.g1_sum_parts_model(9, 1, 1, 0) == 1
    assert dk.g1_wsum_parts_model(5, 130, 1, 0) == 64 and dk.g1_wsum_slices_model(5, 130, 64, 1, 0) == 1
    assert dk.g1_wsum_slices_model(5, 130, 64, 256, 0) == 3 and dk.g1_wsum_slices_model(5, 130, 1, 1, 133) == 130
    assert dk.g1_wsum_slices_model(5, 3, 1, 1, 64) == 3


# ---- (c), (d) the host leg over the case tables; spoiled buffers --------------------------------------------------------
def test_fixed_base_table(host):
    tbl = dk.run_fb_table(host)
    _ok(dk.check_fb_table(tbl, guard=True))
    spoiled = tbl.copy()
    spoiled[300, 20] ^= 1
    assert dk.check_fb_table(spoiled)


def test_fixed_base_products(host):
    case = dk.fb_case()
    res = dk.run_fb(host, case, dk.FB_ALL, 1, 1)
    _ok(dk.check_fb(case, dk.FB_ALL, 1, res))
    _spoiled(dk.check_fb, res, 0, case, dk.FB_ALL, 1)
    _spoiled(dk.check_fb, res, 1, case, dk.FB_ALL, 1)
    _ok(dk.check_fb(case, 257, 0, dk.run_fb(host, case, 257, 1, 0)))


@pytest.mark.parametrize("shape", dk.ROWS_SHAPES)
def test_commitment_rows(host, shape):
    case = dk.rows_case(*shape)
    _ok(dk.check_rows(case, 1, dk.run_rows(host, case)))


def test_commitment_rows_directed(host):
    for case in dk.rows_directed_cases():
        res = dk.run_rows(host, case)
        _ok(dk.check_rows(case, 1, res))
    _spoiled(dk.check_rows, res, 0, case, 1)
    case = dk.rows_case(0, 2, 22)
    _ok(dk.check_rows(case, 0, dk.run_rows(host, case, 0)))


@pytest.mark.parametrize("n", [1, 2, 5, 33])
def test_interpolation(host, n):
    case = dk.interp_case(n)
    res = dk.run_interp(host, case)
    _ok(dk.check_interp(case, 1, res))
    for i in range(3):
        _spoiled(dk.check_interp, res, i, case, 1, at=4 * (2 * (n + 1) * 32) + 3 if i == 1 else 3)  # (job 4 is a random one)
    for with_accept in (0, 1):
        res0 = dk.run_interp0(host, case, with_accept)
        _ok(dk.check_interp0(case, with_accept, res0))
    _spoiled(dk.check_interp0, res0, 0, case, 1)
    statuses = {st for st, _ in case.ref()}
    assert statuses == ({dk.OK, dk.INVALID} if n == 1 else {dk.OK, dk.INVALID, dk.DUPLICATE})


def test_montgomery_matrices(host):
    vals = dk.mont_values()
    res = dk.run_to_mont(host, vals)
    _ok(dk.check_to_mont(vals, -1, res))
    assert dk.check_to_mont(vals, -1, (res[0], 1 - res[1]))
    for degree, variant in [(0, 0), (2, 0), (2, 1), (7, 0)]:
        c = dk.bivar_coeffs(degree, variant)
        _ok(dk.check_to_mont(c, degree, dk.run_to_mont(host, c, degree)))


def test_fr_evaluations(host):
    for n in (0, 1, 4):
        polys, xs, want = dk.poly_evaluate_case(n)
        res = dk.run_poly_evaluate(host, polys, xs)
        _ok(dk.check_fr_rows("poly evaluate n = %d" % n, want, res))
    assert dk.check_fr_rows("spoiled", want, (res[0], res[1] ^ 1))
    for degree, M, variant in dk.BIVAR_ROW_SHAPES:
        c = dk.bivar_coeffs(degree, variant)
        xs = [dk.XS[m % len(dk.XS)] for m in range(M)]
        want = dk.bivar_row_want(degree, c, xs)
        _ok(dk.check_fr_rows("bivar row degree %d" % degree, want, dk.run_bivar_row(host, degree, c, xs)))
        assert variant == 0 or {st for st, _ in want} == {dk.OK, dk.INVALID}


def test_fr_sums(host):
    for n in range(68):
        for weighted in (0, 1):
            case = dk.FrSumCase(n, weighted, n % 3)
            want = case.want()
            _ok(dk.check_fr_rows(case.tag, want, dk.run_fr_sum(host, case)))
            if n >= 2 and case.mode == 2:
                failing = [j for j, (st, _) in enumerate(want) if st != dk.OK]
                assert failing == (list(range(70)) if weighted and n % 2 == 0 else [3, 68]), case.tag
    case = dk.FrSumCase(5, 1, 0)
    _ok(dk.check_fr_rows(case.tag, case.want(), dk.run_fr_sum(host, case, 0), 0))


@pytest.mark.parametrize("n", dk.SUM_NS)
def test_g1_sums(host, n):
    for variant in ("masked", "included"):
        case = dk.sum_case(n, variant)
        first = None
        for parts in HOST_PARTS:
            res = dk.run_sum(host, case, parts)
            _ok(dk.check_sum(case, parts, res))
            first = first or res
            assert dk.same(dk.sum_head(res), dk.sum_head(first)), "%s: parts = %d leaves other bytes" % (case.tag, parts)
        _, st, tb = case.want(9)
        assert (variant == "masked") == (not any(st)) and sum(tb) == (0 if variant == "masked" else (1 if case.k_bad == case.k_mem else 2))
    _spoiled(dk.check_sum, res, 2, case, parts)
    _ok(dk.check_sum(case, 4, dk.run_sum(host, case, 4, 1, 0, 0), 0, 0))


def test_g1_sum_over_first_columns(host):
    for degree in (2, 7):
        case = dk.Column0Case(degree)
        for parts in (1, 2, 4, 3):
            _ok(dk.check_column0_sum(case, parts, dk.run_column0_sum(host, case, parts)))


def test_weight_recoding(host):
    """The recoded words of the host leg by meaning: the 129 sign-aligned columns stand for w (or r - w with `flip`), the flags of
    w = 0 and w >= r are exact, and such weights store no digits.  The device leg must leave these bytes."""
    weights = dk.rec_weights()
    rec = dk.recode_only(host, weights)
    _ok(dk.check_rec(weights, rec))
    spoiled = rec.copy()
    spoiled[9 * 20 + 1] ^= 4
    assert dk.check_rec(weights, spoiled)


HOST_GRID = [(1, 1), (2, 3), (8, 2), (64, 5), (3, 64), (4, 10 ** 6)]


@pytest.mark.parametrize("n,variant,with_sel", [(1, "masked", False), (3, "failing", False), (67, "masked", False), (130, "failing", False),
                                                (5, "masked", True), (5, "failing", True)])
def test_g1_weighted_sums(host, n, variant, with_sel):
    case = dk.wsum_case(n, variant, with_sel)
    first = None
    for parts, slices in HOST_GRID:
        slices = n + 3 if slices == 10 ** 6 else slices
        res = dk.run_wsum(host, case, parts, slices)
        _ok(dk.check_wsum(case, parts, slices, res))
        first = first or res
        assert dk.same(res[:3], first[:3]), "%s: parts = %d, slices = %d leave other final bytes" % (case.tag, parts, slices)
    goods = [case.want_range(j, 0, n)[1] for j in range(5)]
    if variant == "failing":
        assert goods == ([0] * 5 if n >= 5 else [1, 1, 1, 0, 1]), case.tag
    else:
        assert goods == [1] * 5, case.tag
    _spoiled(dk.check_wsum, res, 0, case, parts, slices)


@pytest.mark.parametrize("shape", dk.RLC_SHAPES)
def test_rlc_scalars(host, shape):
    case = dk.RlcCase(*shape)
    res = dk.run_rlc(host, case)
    _ok(dk.check_rlc(case, res))
    _spoiled(dk.check_rlc, res, 0, case)


@pytest.mark.parametrize("shape", dk.RESHARE_SHAPES)
def test_reshare_verdict_chain(host, shape):
    case = dk.reshare_case(*shape)
    res = dk.run_reshare(host, case)
    _ok(dk.check_reshare(case, res))
    for name in ("dup", "part_status", "weights", "status", "out_commit"):
        _spoiled(dk.check_reshare, res, name, case)
    _ok(dk.check_reshare(case, dk.run_reshare(host, case, (False, True))))
    _ok(dk.check_reshare(case, dk.run_reshare(host, case, (True, False))))


def test_reshare_cases_reach_every_verdict():
    seen = {dk.reshare_case(*s).want()["status"] for s in dk.RESHARE_SHAPES}
    assert seen == {dk.OK, dk.NOT_ENOUGH, dk.INVALID, dk.MISMATCH}
    w = dk.reshare_case(257, 6, "mixed").want()
    assert set(w["part_status"]) == {dk.OK, dk.DUPLICATE, dk.INVALID, dk.MISMATCH} and w["dup"][4] == 1 and w["dup"][6] == 0
    w = dk.reshare_case(7, 2, "too few").want()
    assert w["status"] == dk.NOT_ENOUGH and not any(w["used"])
    w = dk.reshare_case(7, 2, "bad old_commit").want()
    assert w["status"] == dk.INVALID and not any(w["part_status"])
    assert (1 << 64) - 1 in dk.reshare_case(7, 2, "all accepted").want()["sel_idx"] and 0 in dk.reshare_case(7, 2, "all accepted").want()["sel_idx"]
