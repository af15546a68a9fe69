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
70 segments of 0 .. 130 records at every power of two of parts up to a wave's worth, and k_rec_gather_keys.  Invalid encodings are ordinary data; after a HIP
error nothing more is launched."""
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
