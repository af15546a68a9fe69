"""GPU leg of the many-point conformance suite (tests/manypoint_conformance.py): the shipped kernels of k_msm.hip (two-stage
linear combinations in G2 and G1) and k_comb.hip (the comb signer), launched by tests/device/manypoint.hip with launch
parameters chosen by the test -- every `parts` / `share` the product's launchers can produce for the shape, and 0 for the
launcher's own choice -- over the case tables the host leg has proven (tests/test_manypoint_host.py).

Per run: output bytes and status bytes against the oracle, the table entries and digit codes the kernels leave in HBM
against the models (affine point, infinity flag, limb range, |value| <= 2.1 p, padding words, the fill beyond the top
column), nothing written for jobs the filter leaves alone / with *need == 0 / in table sets 1 .. B-1 of the shared set, and
the same bytes for every parts / share.  Covered geometry: parts 1 .. 32 (G2) and 1 .. 64 (G1) including the unsplit ladder
kernel, short-scalar mode with nbits = 16 (G2), 32 and 80 (G1), the shared table set, the filter's shapes n = 2, 3, 4,
share = 1 .. 8 of the comb and several workgroups with a ragged tail; the ragged sums of the records verifier (k_rec_*) over
70 segments of 0 .. 130 records at every power of two of parts up to a wave's worth, and k_rec_gather_keys; the PAIRED ragged
sums of the decryption-share verifier (k_rec_*_g1_pair: A_j and -B_j byte for byte in the shipped 32-bit mode and at full
width, half 1's tables and codes behind all of half 0's); the G1 comb of the decryption shares (k_comb_tables_g1 /
k_comb_decrypt) at share = 0 .. 8 over one wave and over 70 ciphertexts, with its 514-entry tables, and k_g1_mul_gather over the
same case; the blame-by-bisection kernels of k_blame.hip through tests/device/manypoint_blame.hip (leaves at n = 1 .. 130 with
leaf numbers across 2^32, the leaf ladders at chosen digits, range sums over 101 ranges of 1 .. 130 leaves at parts = 0 .. 64
and twice that, leaves chained into range sums on the device, blame_sum_parts).  Invalid encodings are ordinary data; after a
HIP error nothing more is launched."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import manypoint_conformance as mp  # noqa: E402

pytestmark = pytest.mark.gpu

_state = {"lib": None, "hip_error": None}


@pytest.fixture(scope="module")
def lib():
    if _state["lib"] is None:
        _state["lib"] = mp.load(mp.build_device(), "mp_")
    return _state["lib"]


def _launch(fn, *args):
    if _state["hip_error"]:
        pytest.fail("not launched after an earlier HIP error: %s" % _state["hip_error"])
    try:
        return fn(*args)
    except mp.HipError as e:
        _state["hip_error"] = str(e)
        raise


def _run_case(lib, case):
    first = None
    for parts in case.parts:
        res = _launch(mp.run_msm, lib, case, parts)
        if first is None or not all((a == b).all() for a, b in zip(res, first)):  # (equal bytes need no second decoding)
            bad = mp.check_msm(case, parts, res)
            assert not bad, "\n".join(bad[:12])
        if first is None:
            first = res
        assert all((a == b).all() for a, b in zip(res, first)), "%s: parts = %d and parts = %d leave different bytes" % (case.tag, parts, case.parts[0])


@pytest.mark.parametrize("n", [8, 9, 13, 68])
def test_g2_msm_full_scalars(lib, n):
    _run_case(lib, mp.msm_case(2, n, 64, 37))


@pytest.mark.parametrize("n,need", [(2, -1), (3, -1), (4, -1), (3, 0), (3, 5)])
def test_g2_msm_filter_shapes(lib, n, need):
    _run_case(lib, mp.filter_case(n, need))


def test_g2_msm_parts_32(lib):
    _run_case(lib, mp.top_case(2))


@pytest.mark.parametrize("n", [1, 5, 64])
def test_g2_msm_short_scalars(lib, n):
    _run_case(lib, mp.msm_case(2, n, 16, 37))


@pytest.mark.parametrize("n", [8, 9, 13, 68])
def test_g1_msm_full_scalars(lib, n):
    _run_case(lib, mp.msm_case(1, n, 128, 70))


def test_g1_msm_parts_64(lib):
    _run_case(lib, mp.top_case(1))


@pytest.mark.parametrize("n,nbits", [(1, 80), (10, 32), (70, 32)])
def test_g1_msm_short_scalars_own_points(lib, n, nbits):
    _run_case(lib, mp.msm_case(1, n, nbits, 70))


@pytest.mark.parametrize("n,variant", [(10, "good"), (10, "job0 even"), (10, "job0 >= r"), (70, "good"), (70, "job0 >= r")])
def test_g1_msm_short_scalars_shared_set(lib, n, variant):
    _run_case(lib, mp.shared_case(n, variant))


@pytest.mark.parametrize("n,B", [(3, 5), (8, 5), (9, 5), (24, 5), (30, 5), (30, 70)])
def test_comb_signer(lib, n, B):
    case = mp.comb_case(n, B)
    first = None
    for share in case.shares:
        res = _launch(mp.run_comb, lib, case, share)
        if first is None or not all((a == b).all() for a, b in zip(res, first)):
            bad = mp.check_comb(case, share, res)
            assert not bad, "\n".join(bad[:12])
        if first is None:
            first = res
        assert all((a == b).all() for a, b in zip(res, first)), "%s: share = %d and share = %d leave different bytes" % (case.tag, share, case.shares[0])


def _run_rec(lib, case):
    first = None
    for parts in case.parts:
        res = _launch(mp.run_rec, lib, case, parts)
        if first is None or not all((a == b).all() for a, b in zip(res, first)):  # (equal bytes need no second decoding)
            bad = mp.check_rec(case, parts, res)
            assert not bad, "\n".join(bad[:12])
        if first is None:
            first = res
        assert all((a == b).all() for a, b in zip(res, first)), "%s: parts = %d and parts = %d leave different bytes" % (case.tag, parts, case.parts[0])


@pytest.mark.parametrize("w,kind", mp.REC_TABLES)
def test_rec_sum(lib, w, kind):
    """The ragged sums (k_rec_tables_* / k_rec_ladder_*) through launch_rec_sum_g1 / _g2: every power of two of parts up to a
    wave's worth, then 3 and twice the maximum (run as parts = 1), all with the same bytes -- outputs, statuses, tables, codes
    and the untouched guards behind them."""
    _run_rec(lib, mp.rec_case(w, kind))


def test_rec_gather_keys(lib):
    got, want = _launch(mp.run_gather, lib)
    assert got == want


@pytest.mark.parametrize("kind", mp.PAIR_TABLES)
def test_rec_sum_pair(lib, kind):
    """The paired ragged sums (k_rec_tables_g1_pair / k_rec_ladder_g1_pair) through launch_rec_sum_g1_pair: out[2 j] = A_j and
    out[2 j + 1] = -B_j byte for byte (an error common to both halves cancels in the product check of the verifier, not here), the
    statuses, half 0's and half 1's tables and codes at their chunk offsets, the guard chunk and guard rows; parts = 1 .. 64, then
    3 and 128 (run as parts = 1), all with the same bytes."""
    case = mp.pair_case(kind)
    mp.sweep(lib, case, mp.run_rec_pair, mp.check_rec_pair, case.parts, "parts", _launch)


@pytest.mark.parametrize("n,B", mp.COMB1_SHAPES)
def test_comb_g1(lib, n, B):
    """The G1 comb of the decryption shares (k_comb_tables_g1 / k_comb_decrypt): share = 0 (launch_comb_decrypt, which takes one
    holder per lane at these sizes) and every forced share = 1 .. 8 -- the wave's holder loop, lanes with fewer holders than their
    wave's longest, lanes past the end -- leave the same outputs, statuses, ok bytes and 66 KB tables, all equal to the model."""
    case = mp.comb1_case(n, B)
    mp.sweep(lib, case, mp.run_comb1, mp.check_comb1, case.shares, "share", _launch)


def test_g1_mul_gather_leaves_the_bytes_of_the_comb(lib):
    """k_g1_mul_gather (one arena ladder per share, 630 lanes with a ragged last wave) over the comb's B = 70, n = 9 case: the
    comb's output and status bytes, the guards untouched, every arena slot free again afterwards."""
    case = mp.comb1_case(9, 70)
    out, status = _launch(mp.run_g1_mul_gather, lib, case)
    bad = mp.check_comb1_out(case, case.tag + " gather", out, status)
    assert not bad, "\n".join(bad[:12])
    comb = _launch(mp.run_comb1, lib, case, 8)
    assert (out == comb[0]).all() and (status == comb[1]).all()


# ---- blame by bisection (k_blame.hip), through tests/device/manypoint_blame.hip ----
@pytest.fixture(scope="module")
def blame():
    if _state.get("blame") is None:
        _state["blame"] = mp.load_blame(mp.build_device_blame(), "mp_")
    return _state["blame"]


@pytest.mark.parametrize("w,shape", [(w, s) for w in (1, 2) for s in mp.LEAVES_SHAPES])
def test_blame_leaves(blame, w, shape):
    """launch_blame_seed + launch_blame_leaves with a fresh arena: the seed, every leaf decoded from its raw words ([r_i] P_i, Z = 0
    for a dead slot, limb range, |value| <= 2.1 p, padding words, the c0 / c1 rows), the live bytes, the guard row and byte, every
    arena slot free again -- ragged last waves, leaf numbers across 2^32, the three forms of period / live."""
    case = mp.leaves_case(w, *shape)
    bad = mp.check_blame_leaves(case, _launch(mp.run_blame_leaves, blame, case))
    assert not bad, "\n".join(bad[:12])


@pytest.mark.parametrize("w", [1, 2])
def test_blame_ladder_at_chosen_digits(blame, w):
    """blame_leaf_g1 / blame_leaf_g2 at digits ChaCha20 gives with probability 2^-16 or less: zeros, all ones, k2 = 0."""
    case = mp.ladder_case(w)
    bad = mp.check_blame_ladder(case, _launch(mp.run_blame_ladder, blame, case))
    assert not bad, "\n".join(bad[:12])


@pytest.mark.parametrize("w", [1, 2])
def test_blame_range_sum(blame, w):
    """k_blame_range_sum through launch_blame_range_sum over leaves written by the test: parts = 0 (blame_sum_parts), every power
    of two up to a wave's worth -- most lanes of a short range are then empty and run masked trips only --, then 3 and twice the
    maximum (run as 1): the oracle's bytes for every item, the guard rows, the same bytes at every parts."""
    case = mp.range_case(w)
    mp.sweep(blame, case, mp.run_blame_range, mp.check_blame_range, mp.BLAME_PARTS[w], "parts", _launch)


@pytest.mark.parametrize("w", [1, 2])
def test_blame_leaves_then_range_sum(blame, w):
    """k_blame_leaves -> k_blame_range_sum in one entry, over the leaves where the first kernel left them (n = 130, leaf numbers
    across 2^32)."""
    case = mp.chain_case(w)
    mp.sweep(blame, case, mp.run_blame_chain, mp.check_blame_chain, case.parts, "parts", _launch)


def test_blame_sum_parts(blame):
    for w, n_items, longest, cus in mp.SUM_PARTS_TABLE:
        got = blame["sum_parts"](w - 1, n_items, longest, cus)
        what = (w, n_items, longest, cus, got)
        assert got == mp.blame_sum_parts_model(w, n_items, longest, cus), what
        assert got >= 1 and got & (got - 1) == 0 and got <= mp.MAX_PARTS[w] and (got == 1 or 2 * got <= longest), what
